"""GPU: the photometric training augmentation (csrc/photometric.h behind the warp: og_warp_affine_photo_batch_u8; csrc/jpeg_sim.hip:
og_jpeg_roundtrip_batch_u8; og_affine_joints_jitter_f32; transforms.DeviceAugment with PhotoParams; train_dist's flags).

Every kernel case asserts equality with the numpy restatement of the specification (tests/photometric_common.py on top of
tests/augment_common.py): integer arithmetic, and fp32 operations that are each correctly rounded in a fixed order on both sides, so no
tolerance applies.  Shapes are tiny: the three sources of augment_common in one launch, destination squares of 64 and 50 pixels (50 is
neither a multiple of the warp's tile nor of 4, and leaves a partial MCU of 2 x 2 pixels on both axes)."""
import ctypes as C
import json
import math
import random

import numpy as np
import pytest
import torch

import augment_common as ac
import photometric_common as pc
from offsetguided_amd import _lib, transforms
from offsetguided_amd.models import networks

pytestmark = pytest.mark.gpu
SIDES = (64, 50)
SENTINEL = -77.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sources(dev):
    images, _ = ac.source_images()
    raw = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(dev)
    return images, raw


@pytest.fixture(scope="module")
def warped(sources):
    """S -> (D rows, [the restated warp of each source]) for the magnifying case: the crop is full of image.  Computed once."""
    out = {}
    for S in SIDES:
        D = [ac.inverse_rows(m) for m in ac.fixed_cases(S)['scale2_stretch']]
        out[S] = (D, [ac.warp_u8(im, D[i], S, ac.BORDER) for i, im in enumerate(sources[0])])
    return out


def _tables(sizes):
    n = len(sizes)
    offs, hw4, o = (C.c_long * n)(), (C.c_int * (4 * n))(), 0
    for i, (h, w) in enumerate(sizes):
        offs[i] = o
        hw4[4 * i:4 * i + 4] = [h, w, 0, 0]
        o += h * w * 3
    return offs, hw4


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _i32(values):
    return np.ascontiguousarray(np.asarray(values, np.int32))


def _photo_warp(dev, raw, D, S, table, offs=None, hw4=None, plain=False):
    """og_warp_affine_photo_batch_u8 (or the plain entry) -> (status, fp32 NCHW, uint8 NHWC), both pre-filled with a sentinel."""
    lib = _lib.load()
    n = len(D)
    if offs is None:
        offs, hw4 = _tables(ac.SIZES)
    D = np.ascontiguousarray(np.asarray(D, np.float64).reshape(n, 6))
    out = torch.full((n, 3, S, S), SENTINEL, dtype=torch.float32, device=dev)
    u8 = torch.full((n, S, S, 3), 7, dtype=torch.uint8, device=dev)
    head = (_lib.ptr(raw), offs, hw4, n, D.ctypes.data_as(C.c_void_p), S, (C.c_ubyte * 3)(*ac.BORDER), _f3(ac.MEAN), _f3(ac.STD),
            _lib.ptr(out), _lib.ptr(u8))
    if plain:
        return lib.og_warp_affine_batch_u8(*head, _lib.stream_ptr(dev)), out, u8
    table = _i32(table) if table is not None else None
    return lib.og_warp_affine_photo_batch_u8(*head, table.ctypes.data_as(C.c_void_p) if table is not None else None,
                                             _lib.stream_ptr(dev)), out, u8


def _jpeg(dev, u8, out, selected, quality, table):
    lib = _lib.load()
    n, S = u8.shape[0], u8.shape[1]
    table = _i32(table) if table is not None else None
    return lib.og_jpeg_roundtrip_batch_u8(_lib.ptr(u8), n, S, (C.c_int * max(len(selected), 1))(*selected), len(selected), quality,
                                          table.ctypes.data_as(C.c_void_p) if table is not None else None, _f3(ac.MEAN), _f3(ac.STD),
                                          _lib.ptr(out), _lib.stream_ptr(dev))


def _norm(rgb):
    return torch.from_numpy(pc.normalize(rgb))


# ---------------------------------------------------------------------------------------------------------------- warp + epilogue
@pytest.mark.parametrize('S', SIDES)
def test_mixed_modes_in_one_launch(dev, sources, warped, S):
    """none / tint (then a JPEG round trip of that image) / gray: the warp's launch, then the JPEG pass on image 1 alone."""
    D, ref = warped[S]
    rc, out, u8 = _photo_warp(dev, sources[1], D, S, pc.PHOTO_MIX)
    assert rc == _lib.OG_OK
    got = out.cpu()
    for i in range(3):
        assert np.array_equal(u8[i].cpu().numpy(), ref[i]), f'image {i}: out_u8 is the warped value itself'
        assert torch.equal(got[i], _norm(pc.epilogue(ref[i], pc.PHOTO_MIX[i]))), f'image {i}: mode {pc.PHOTO_MIX[i][0]}'
    assert not torch.equal(got[1], _norm(ref[1])) and not torch.equal(got[2], _norm(ref[2]))
    assert _jpeg(dev, u8, out, [1], 50, pc.PHOTO_MIX) == _lib.OG_OK
    after = out.cpu()
    assert torch.equal(after[0], got[0]) and torch.equal(after[2], got[2])
    assert torch.equal(after[1], _norm(pc.epilogue(pc.jpeg_roundtrip(ref[1], 50), pc.PHOTO_MIX[1])))
    assert not torch.equal(after[1], got[1])


@pytest.mark.parametrize('S', SIDES)
def test_tint_corners(dev, sources, warped, S):
    """The eight corners of the reference's delta box (+-10, +-40, +-30) and the zero tint, three per launch."""
    D, ref = warped[S]
    for first in range(0, 9, 3):
        table = [(pc.MODE_TINT,) + pc.TINT_CORNERS[first + i] for i in range(3)]
        rc, out, _ = _photo_warp(dev, sources[1], D, S, table)
        assert rc == _lib.OG_OK
        got = out.cpu()
        for i in range(3):
            exp = pc.tint(ref[i], *pc.TINT_CORNERS[first + i])
            diff = np.argwhere((got[i] != _norm(exp)).numpy().any(axis=0))
            assert torch.equal(got[i], _norm(exp)), f'deltas {pc.TINT_CORNERS[first + i]}, image {i}: first (row, col) {diff[:5].tolist()}'


@pytest.mark.parametrize('S', SIDES)
def test_tint_and_gray_together(dev, sources, warped, S):
    D, ref = warped[S]
    table = [(3, -10, 40, -30), (3, 0, 0, 0), (2, 9, 9, 9)]                # (gray alone ignores the deltas)
    rc, out, _ = _photo_warp(dev, sources[1], D, S, table)
    assert rc == _lib.OG_OK
    got = out.cpu()
    for i in range(3):
        exp = pc.epilogue(ref[i], table[i])
        assert (exp[..., 0] == exp[..., 1]).all() and torch.equal(got[i], _norm(exp)), i


@pytest.mark.parametrize('S', SIDES)
def test_all_modes_off_equals_the_plain_entry(dev, sources, warped, S):
    D, ref = warped[S]
    rc, out, u8 = _photo_warp(dev, sources[1], D, S, np.zeros((3, 4), np.int32))
    rc2, out2, u82 = _photo_warp(dev, sources[1], D, S, None, plain=True)
    assert rc == rc2 == _lib.OG_OK and torch.equal(out, out2) and torch.equal(u8, u82)
    assert torch.equal(out[0].cpu(), _norm(ref[0]))


# ------------------------------------------------------------------------------------------------------------------------- JPEG
@pytest.mark.parametrize('quality', (10, 50, 95))
@pytest.mark.parametrize('S', SIDES)
def test_jpeg_roundtrip(dev, warped, S, quality):
    """Images 0 and 2 selected, no epilogue (a null table): bit for bit the restatement; image 1 keeps its sentinel."""
    _, ref = warped[S]
    u8 = torch.from_numpy(np.stack(ref)).to(dev)
    out = torch.full((3, 3, S, S), SENTINEL, dtype=torch.float32, device=dev)
    assert _jpeg(dev, u8, out, [0, 2], quality, None) == _lib.OG_OK
    got = out.cpu()
    assert bool((got[1] == SENTINEL).all())
    for i in (0, 2):
        exp = pc.jpeg_roundtrip(ref[i], quality)
        diff = np.argwhere((got[i] != _norm(exp)).numpy().any(axis=0))
        assert torch.equal(got[i], _norm(exp)), f'image {i}: {len(diff)} pixels differ, first (row, col) {diff[:5].tolist()}'
        assert not np.array_equal(exp, ref[i])
    assert _jpeg(dev, u8, out, [], quality, None) == _lib.OG_OK                    # nothing selected: nothing happens
    assert torch.equal(out.cpu(), got)


def test_more_images_than_one_launch_carries(dev, sources):
    """35 images, all with a JPEG round trip: the descriptor tables of the warp and of the JPEG pass hold 32 each."""
    images, raw = sources
    S, n = 50, 35
    rs = np.random.RandomState(2)
    D = [ac.inverse_rows(np.array([[1.5, 0, rs.uniform(-9, 9)], [0, 1.5, rs.uniform(-9, 9)], [0, 0, 1.]])) for _ in range(n)]
    offs, hw4 = _tables(ac.SIZES)
    offs_n, hw4_n = (C.c_long * n)(), (C.c_int * (4 * n))()
    for i in range(n):
        offs_n[i] = offs[i % 3]
        hw4_n[4 * i:4 * i + 4] = hw4[4 * (i % 3):4 * (i % 3) + 4]
    table = [(i % 4, (i % 21) - 10, (5 * i) % 81 - 40, (7 * i) % 61 - 30) for i in range(n)]
    rc, out, u8 = _photo_warp(dev, raw, D, S, table, offs_n, hw4_n)
    assert rc == _lib.OG_OK
    first = out.cpu()
    assert _jpeg(dev, u8, out, list(range(n))[::-1], 50, table) == _lib.OG_OK      # (any order)
    second = out.cpu()
    for i in (0, 1, 2, 3, 31, 32, 33, 34):
        ref = ac.warp_u8(images[i % 3], D[i], S, ac.BORDER)
        assert np.array_equal(u8[i].cpu().numpy(), ref), i
        assert torch.equal(first[i], _norm(pc.epilogue(ref, table[i]))), i
        assert torch.equal(second[i], _norm(pc.epilogue(pc.jpeg_roundtrip(ref, 50), table[i]))), i


def test_argument_errors_are_status_codes(dev, sources, warped):
    """Host-side refusals only: nothing is launched, the outputs keep their sentinel."""
    lib = _lib.load()
    S = 64
    D, ref = warped[S]
    ok = np.zeros((3, 4), np.int32)
    outs = []

    def warp(table):
        rc, out, u8 = _photo_warp(dev, sources[1], D, S, table)
        outs.extend([out, u8])
        return rc

    assert warp(None) == _lib.OG_EINVAL and b'null pointer' in lib.og_last_error()
    for col, bad in ((0, 4), (0, -1), (1, 181), (2, -256), (3, 256)):
        table = ok.copy()
        table[1, col] = bad
        assert warp(table) == _lib.OG_EINVAL and b'image 1' in lib.og_last_error(), (col, bad)
    far = [D[0], np.array([[2.0 ** 14, 0, 0], [0, 1, 0.]]), D[2]]
    rc, out, u8 = _photo_warp(dev, sources[1], far, S, ok)
    outs.extend([out, u8])
    assert rc == _lib.OG_EINVAL and b'2^20' in lib.og_last_error()
    u8 = torch.from_numpy(np.stack(ref)).to(dev)
    out = torch.full((3, 3, S, S), SENTINEL, dtype=torch.float32, device=dev)
    for quality in (0, 101):
        assert _jpeg(dev, u8, out, [0], quality, None) == _lib.OG_EINVAL and b'quality' in lib.og_last_error()
    for sel in ([3], [-1], [0, 1, 7]):
        assert _jpeg(dev, u8, out, sel, 50, None) == _lib.OG_EINVAL and b'selected' in lib.og_last_error()
    bad = ok.copy()
    bad[2, 0] = 8
    assert _jpeg(dev, u8, out, [2], 50, bad) == _lib.OG_EINVAL and b'image 2' in lib.og_last_error()
    assert _jpeg(dev, u8, out, [0], 50, bad) == _lib.OG_OK                         # only the selected images' descriptors count
    assert lib.og_jpeg_roundtrip_batch_u8(_lib.ptr(u8), 3, S, (C.c_int * 1)(0), -1, 50, None, _f3(ac.MEAN), _f3(ac.STD), _lib.ptr(out),
                                          _lib.stream_ptr(dev)) == _lib.OG_EINVAL
    assert lib.og_jpeg_roundtrip_batch_u8(None, 3, S, (C.c_int * 1)(0), 1, 50, None, _f3(ac.MEAN), _f3(ac.STD), _lib.ptr(out),
                                          _lib.stream_ptr(dev)) == _lib.OG_EINVAL
    torch.cuda.synchronize()
    assert bool((out[1:] == SENTINEL).all()) and not bool((out[0] == SENTINEL).any())
    for t in outs:
        assert bool((t == (SENTINEL if t.dtype == torch.float32 else 7)).all())


# ----------------------------------------------------------------------------------------------------------------------- jitter
def _joints_call(dev, joints, n_persons, M, flips, scales, S_w, S_h, jitter=None):
    """jitter = (noise (N,P,K,2), gate, eps, shift) -> og_affine_joints_jitter_f32, else the plain entry; -> (status, out on the host)."""
    lib = _lib.load()
    n, P, K, _ = joints.shape
    jd, nd = torch.from_numpy(joints).to(dev), torch.from_numpy(n_persons).to(dev)
    out = torch.full(joints.shape, SENTINEL, dtype=torch.float32, device=dev)
    M = np.ascontiguousarray(np.asarray(M, np.float64).reshape(n, 6))
    head = (_lib.ptr(jd), _lib.ptr(nd), n, P, K, M.ctypes.data_as(C.c_void_p), (C.c_int * n)(*flips), (C.c_double * n)(*scales),
            float(S_w), float(S_h), (C.c_int * 8)(*ac.LEFT), (C.c_int * 8)(*ac.RIGHT), 8)
    if jitter is None:
        rc = lib.og_affine_joints_f32(*head, _lib.ptr(out), _lib.stream_ptr(dev))
    else:
        noise, gate, eps, shift = jitter
        nz = torch.from_numpy(np.ascontiguousarray(noise, np.float32)).to(dev) if noise is not None else None
        rc = lib.og_affine_joints_jitter_f32(*head, _lib.ptr(nz) if nz is not None else None, (C.c_int * n)(*gate), (C.c_float * n)(*eps),
                                             (C.c_float * n)(*shift), _lib.ptr(out), _lib.stream_ptr(dev))
    return rc, out.cpu()


def test_jitter_equals_the_restatement_on_the_fixture(dev):
    """The warp fixture's 64 cases as one batch (two launches' worth of descriptors), every third image ungated, eps and shift per
    image: bit for bit the restatement; padding rows keep their sentinel; an ungated image equals the plain entry; visibility is the
    plain entry's (no second test)."""
    z = np.load(ac.GOLDEN)
    joints, n_persons, params = z['joints'].copy(), z['n_persons'], z['params']
    for c in range(64):
        joints[c, n_persons[c]:] = 123.25
    flips = [int(p[0]) for p in params]
    scales = [math.sqrt((p[3] * p[2]) * (p[4] * p[2])) for p in params]
    noise = np.random.RandomState(8).uniform(0, 1, joints.shape[:3] + (2,)).astype(np.float32)
    gate = [int(c % 3 != 1) for c in range(64)]
    eps = [(0.5, 0.25, 3.0, 0.1)[c % 4] for c in range(64)]
    shift = [(0.0, 1.0, -0.3)[c % 3 if c % 2 else 0] for c in range(64)]
    rc, plain = _joints_call(dev, joints, n_persons, z['mat'][:, :2], flips, scales, 512, 512)
    rc2, got = _joints_call(dev, joints, n_persons, z['mat'][:, :2], flips, scales, 512, 512, (noise, gate, eps, shift))
    assert rc == rc2 == _lib.OG_OK
    moved = 0
    for c in range(64):
        n = int(n_persons[c])
        ref = ac.affine_joints(joints[c], n, z['mat'][c][:2], flips[c], scales[c], 512, 512)
        assert torch.equal(plain[c], torch.from_numpy(ref)), c
        if gate[c]:
            ref = pc.jitter_joints(ref, n, noise[c], eps[c], shift[c])
            moved += int(not torch.equal(got[c], plain[c]))
        else:
            assert torch.equal(got[c], plain[c]), c
        assert torch.equal(got[c], torch.from_numpy(ref)), c
        assert bool((got[c, n:] == 123.25).all()) and torch.equal(got[c, :, :, 2:], plain[c, :, :, 2:]), c
    assert moved >= 40
    rc, _ = _joints_call(dev, joints, n_persons, z['mat'][:, :2], flips, scales, 512, 512, (None, gate, eps, shift))
    assert rc == _lib.OG_EINVAL and b'null pointer' in _lib.load().og_last_error()


# ------------------------------------------------------------------------------------------------------------- DeviceAugment
def test_device_augment_with_every_step_on(dev, sources):
    """All four probabilities 1: the call queues without a host-device sync and equals the entry points called by hand with the draws
    it reports, and so the restatement; PhotoParams() changes nothing."""
    images, raw = sources
    S = 50
    rs = np.random.RandomState(4)
    joints = np.zeros((3, 3, 17, 4), np.float32)
    for i, (h, w) in enumerate(ac.SIZES):
        joints[i, :, :, 0] = np.round(rs.uniform(2, w - 3, (3, 17)) * 4) / 4
        joints[i, :, :, 1] = np.round(rs.uniform(2, h - 3, (3, 17)) * 4) / 4
    joints[:, :, :, 2] = (rs.uniform(0, 1, (3, 3, 17)) > 0.2) * 2
    joints[:, :, :, 3] = rs.uniform(1, 9, (3, 3, 17))
    n_persons = np.array([3, 1, 0], np.int32)
    np_rng = np.random.RandomState(0)
    photo = transforms.PhotoParams(tint_prob=1, gray_prob=1, jpeg_prob=1, jpeg_quality=30, jitter_prob=1, jitter_epsilon=0.75, jitter_shift=1)
    aug = transforms.DeviceAugment(S, transforms.AugParams(max_translate=8, min_scale=1.5), device=dev, photo_params=photo, np_rng=np_rng)
    for _ in range(3):                                                    # allocator, the three pinned staging buffers, library warm-up
        aug(images, joints, n_persons, rng=random.Random(1))
    torch.cuda.synchronize()
    np_rng.seed(5)
    torch.manual_seed(9)
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        out, jout, mout, mats = aug(images, joints, n_persons, rng=random.Random(11))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    # the draws: the seven of every image first, then per image four gates; deltas and noise from their own generators
    rng, twin_np = random.Random(11), np.random.RandomState(5)
    params = [aug.transform.draw(rng) for _ in range(3)]
    assert params == aug.last_params and mout is None
    torch.manual_seed(9)
    exp_photo = transforms.draw_photo(photo, n_persons, 17, rng, twin_np)
    assert len(aug.last_photo) == 3
    for d, e in zip(aug.last_photo, exp_photo):
        assert d['tint'] == e['tint'] and d['jpeg'] == e['jpeg'] == 30 and d['gray'] is True and np.array_equal(d['jitter'], e['jitter'])
    assert [d['jitter'].shape[0] for d in aug.last_photo] == [3, 1, 0]
    # by hand
    D = [transforms.inverse_rows(m, S) for m in mats]
    table = transforms.photo_table(aug.last_photo)
    assert (table[:, 0] == 3).all()
    rc, o2, u8 = _photo_warp(dev, raw, D, S, table)
    assert rc == _lib.OG_OK and _jpeg(dev, u8, o2, [0, 1, 2], 30, table) == _lib.OG_OK
    assert out.shape == (3, 3, S, S) and torch.equal(out, o2)
    for i in range(3):
        ref = pc.epilogue(pc.jpeg_roundtrip(ac.warp_u8(images[i], D[i], S, ac.BORDER), 30), table[i])
        assert torch.equal(out[i].cpu(), _norm(ref)), i
    flips = [int(p[0]) for p in params]
    scales = [math.sqrt((p[3] * p[2]) * (p[4] * p[2])) for p in params]
    noise = np.zeros((3, 3, 17, 2), np.float32)
    for i in range(3):
        noise[i, :n_persons[i]] = aug.last_photo[i]['jitter']
    rc, j2 = _joints_call(dev, joints, n_persons, mats[:, :2], flips, scales, S, S, (noise, [1] * 3, [0.75] * 3, [1.0] * 3))
    ref = np.stack([pc.jitter_joints(ac.affine_joints(joints[i], int(n_persons[i]), mats[i][:2], flips[i], scales[i], S, S),
                                     int(n_persons[i]), noise[i], 0.75, 1) for i in range(3)])
    assert rc == _lib.OG_OK and torch.equal(jout.cpu(), j2) and torch.equal(j2, torch.from_numpy(ref))
    # every probability 0: no draw, the plain launches
    plain = transforms.DeviceAugment(S, transforms.AugParams(max_translate=8, min_scale=1.5), device=dev)
    off = transforms.DeviceAugment(S, transforms.AugParams(max_translate=8, min_scale=1.5), device=dev, photo_params=transforms.PhotoParams())
    a, b = plain(images, joints, n_persons, rng=random.Random(11)), off(images, joints, n_persons, rng=random.Random(11))
    assert off.last_photo is None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[3], mats)
    assert not torch.equal(a[0], out)


# ---------------------------------------------------------------------------------------------------------------- train_dist
def test_train_dist_photometric_flags(dev, tmp_path, monkeypatch, capsys):
    """Two timed steps of train_dist --bench --augment --color-tint-prob 1 --jpeg-prob 1 at 256 x 256, batch 2: finite losses, and the
    line names the probabilities.  (256: the size of every GPU training test of the Hourglass-104.)"""
    from offsetguided_amd import train_dist
    monkeypatch.setattr(networks.torch, 'save', lambda data, path: None)
    seen = []
    real_step = train_dist.train_step

    def spy(model, criterion, optimizer, images, annos, *a, **k):
        loss, parts = real_step(model, criterion, optimizer, images, annos, *a, **k)
        seen.append((bool(torch.isfinite(images).all()), float(loss)))
        return loss, parts

    monkeypatch.setattr(train_dist, 'train_step', spy)
    train_dist.main(['--no-pretrain', '--square-length', '256', '--batch-size', '2', '--checkpoint-path', str(tmp_path), '--augment',
                     '--color-tint-prob', '1', '--jpeg-prob', '1', '--bench', '--bench-steps', '2', '--bench-warmup', '1'])
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith('{')][-1])
    assert line['augment_us'] > 0 and line['steps'] == 2 and line['value'] > 0
    assert line['photo_probs'] == {'color_tint': 1.0, 'gray': 0.0, 'jpeg': 1.0, 'jpeg_quality': 50, 'annotation_jitter': 0.0}
    assert len(seen) == 3 and all(ok and np.isfinite(loss) for ok, loss in seen)
