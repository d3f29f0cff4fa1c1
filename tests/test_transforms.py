"""Input-side transforms (the part without cv2): CenterPad + ToTensor + Normalize in one HIP pass against
the same arithmetic in torch on the CPU (torchvision's ToTensor / Normalize are `div(255)`, `sub_(mean).div_(std)`;
torchvision.transforms.functional.pad with a colour fill is a constant border)."""
import os

import numpy as np
import pytest
import torch

from offsetguided_amd import transforms
from offsetguided_amd.config import data_mean, data_std


def test_center_pad_ltrb_matches_reference_formula():
    # transforms/pad.py:40-55 on a few sizes (odd differences put the extra pixel right / down)
    assert transforms.center_pad_ltrb(640, 427, 640, 640) == (0, 106, 0, 107)
    assert transforms.center_pad_ltrb(480, 640, 640, 640) == (80, 0, 80, 0)
    assert transforms.center_pad_ltrb(333, 501, 640, 640) == (153, 69, 154, 70)
    assert transforms.center_pad_ltrb(640, 640, 640, 640) == (0, 0, 0, 0)


@pytest.mark.gpu
def test_center_pad_normalize_bit_exact():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((427, 640), (640, 480), (501, 333), (640, 640), (1, 1))]
    metas = [{'offset': np.array([0.0, 0.0]), 'valid_area': np.array([0.0, 0.0, im.shape[1], im.shape[0]])} for im in images]
    op = transforms.CenterPadNormalize(640)
    out = op(images, metas).cpu()
    mean, std = torch.tensor(data_mean).view(3, 1, 1), torch.tensor(data_std).view(3, 1, 1)
    for im, got, meta in zip(images, out, metas):
        h, w = im.shape[:2]
        left, top, right, bottom = transforms.center_pad_ltrb(w, h, 640, 640)
        canvas = np.empty((640, 640, 3), np.uint8)
        canvas[:] = np.array(transforms.pad.FILL, np.uint8)
        canvas[top:top + h, left:left + w] = im
        ref = (torch.from_numpy(canvas).permute(2, 0, 1).float().div(255) - mean) / std
        assert torch.equal(got, ref)
        assert tuple(meta['offset']) == (-left, -top) and tuple(meta['valid_area'][:2]) == (left, top)
        assert tuple(meta['width_height']) == (640, 640)


def test_rescale_size_and_meta_follow_the_reference_formulas():
    # transforms/scale.py:91-97: the long edge becomes long_edge, the other one int(edge * s)
    assert transforms.rescale_size(640, 427, 640) == (640, 427)
    assert transforms.rescale_size(500, 375, 640) == (640, 480)
    assert transforms.rescale_size(375, 500, 640) == (480, 640)
    assert transforms.rescale_size(333, 1000, 640) == (213, 640)
    assert transforms.rescale_size(500, 375, 640, fixed_height=True) == (853, 640)
    meta = transforms.initial_meta(500, 375, image_id=7)
    anns = np.zeros((1, 17, 4), np.float32)
    anns[0, :, 0], anns[0, :, 1], anns[0, :, 3] = 100.0, 50.0, 8.0
    m2, a2 = transforms.rescale_meta(meta, anns, 500, 375, 640, 480)
    sx, sy = 639 / 499, 479 / 374                                    # (w' - 1) / (w - 1), transforms/scale.py:37-38
    assert np.allclose(m2['scale'], [sx, sy]) and np.allclose(m2['offset'], [0, 0]) and tuple(m2['width_height']) == (640, 480)
    assert np.allclose(m2['valid_area'], [0, 0, 500 * sx, 375 * sy])
    assert np.allclose(a2[0, 0], [100 * sx, 50 * sy, 0, 8 * np.sqrt(sx * sy)], rtol=1e-6)
    assert tuple(meta['scale']) == (1.0, 1.0) and anns[0, 0, 0] == 100.0       # inputs untouched
    # ... and annotations_inverse undoes rescale + centre pad
    from offsetguided_amd.evaluate import annotations_inverse
    m2['offset'] = m2['offset'] - np.array([0.0, 80.0])
    kp = np.zeros((1, 17, 6), np.float32)
    kp[0, :, 0], kp[0, :, 1], kp[0, :, 3] = 100 * sx, 50 * sy + 80, 8 * np.sqrt(sx * sy)
    back = annotations_inverse(kp, m2)
    assert np.allclose(back[0, 0, :2], [100, 50], atol=1e-4) and np.allclose(back[0, 0, 3], 8, atol=1e-5)


def test_resize_restatement_properties():
    """The CPU restatement of cv2.resize(INTER_CUBIC) (parity with cv2 unpinned): identity at equal size, constant images
    stay constant, a x2 enlargement of a ramp stays monotone inside, replicated borders."""
    import oracle
    rng = np.random.default_rng(1)
    im = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert (oracle.resize_cubic_u8(im, 9, 13) == im).all()
    assert (oracle.resize_cubic_u8(np.full((7, 5, 3), 201, np.uint8), 19, 11) == 201).all()
    ramp = np.tile(np.arange(0, 240, 12, dtype=np.uint8)[None, :, None], (6, 1, 3))
    up = oracle.resize_cubic_u8(ramp, 12, 40).astype(int)
    assert (np.diff(up[3, :, 0]) >= 0).all() and up[3, 0, 0] <= 2 and up[3, -1, 0] >= 225
    down = oracle.resize_cubic_u8(rng.integers(0, 256, (64, 48, 3), dtype=np.uint8), 21, 16)
    assert down.shape == (21, 16, 3)


@pytest.mark.gpu
def test_resize_and_fused_chain_bit_exact_vs_restatement():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    import oracle
    rng = np.random.default_rng(2)
    cases = [((427, 640), 640), ((640, 480), 640), ((375, 500), 640), ((1000, 333), 640), ((31, 17), 128), ((640, 640), 640),
             ((240, 320), 512)]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w), _ in cases]
    mean, std = torch.tensor(data_mean).view(3, 1, 1), torch.tensor(data_std).view(3, 1, 1)
    for im, ((h, w), T) in zip(images, cases):
        tw, th = transforms.rescale_size(w, h, T)
        ref = oracle.resize_cubic_u8(im, th, tw)
        got = transforms.resize_cubic(im, th, tw).cpu().numpy()
        assert (got == ref).all(), (h, w, T)
        pre = transforms.EvalPreprocess(T)
        out, metas = pre([im], image_ids=[5])
        left, top, _, _ = transforms.center_pad_ltrb(tw, th, T, T)
        canvas = np.empty((T, T, 3), np.uint8)
        canvas[:] = np.array(transforms.pad.FILL, np.uint8)
        canvas[top:top + th, left:left + tw] = ref
        expect = (torch.from_numpy(canvas).permute(2, 0, 1).float().div(255) - mean) / std
        assert torch.equal(out[0].cpu(), expect)
        sx, sy = (tw - 1) / (w - 1), (th - 1) / (h - 1)
        assert np.allclose(metas[0]['scale'], [sx, sy]) and np.allclose(metas[0]['offset'], [-left, -top])
        assert metas[0]['image_id'] == 5
    # --fixed-height chain: RescaleHighAbsolute + RightDownPad to a multiple of 128, image in the top-left corner
    im = images[2]                                               # 375 x 500 -> 640 x 853 -> padded 640 x 896
    out, metas = transforms.EvalPreprocess(640, fixed_height=True)([im])
    assert transforms.rescale_size(500, 375, 640, fixed_height=True) == (853, 640) and out.shape == (1, 3, 640, 896)
    canvas = np.empty((640, 896, 3), np.uint8)
    canvas[:] = np.array(transforms.pad.FILL, np.uint8)
    canvas[:640, :853] = oracle.resize_cubic_u8(im, 640, 853)
    assert torch.equal(out[0].cpu(), (torch.from_numpy(canvas).permute(2, 0, 1).float().div(255) - mean) / std)
    assert np.allclose(metas[0]['offset'], [0, 0]) and tuple(metas[0]['width_height']) == (896, 640)
    with pytest.raises(AssertionError):
        transforms.EvalPreprocess(640, fixed_height=True)([images[2], images[0]])   # different padded widths in one batch
    pre = transforms.EvalPreprocess(640)
    for _ in range(3):                                           # a batch of mixed sizes, staging buffers reused
        out, metas = pre(images[:4])
        assert out.shape == (4, 3, 640, 640) and len(metas) == 4
        single, _ = pre([images[2]])
        assert torch.equal(out[2], single[0])


@pytest.mark.gpu
def test_batched_input_chain_equals_per_image_launches():
    """og_rescale_pad_normalize_batch_u8 (one launch per batch, evaluate.py:157-182) == og_rescale_pad_normalize_u8 per image, bit for
    bit: mixed sizes incl. a 4.7x reduction (3000 x 2000 -> 640 x 426: the footprint estimate is 308 x 26 x 3 = 24 024 bytes, still
    the LDS path), a 5.2x one (3300 x 2200: 338 x 28 x 3 bytes, the direct path; tests/input_chain_common.takes_lds restates the
    decision) and an enlargement, both paddings, and more images than one launch's descriptor table holds (64).  Both entries share the
    tile function: what holds them to an independent reference is tests/test_gpu_input_chain.py."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    import ctypes as C
    from offsetguided_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(11)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    mean, std, fill = f3(data_mean), f3(data_std), f3(transforms.pad.FILL)
    for T, fixed, sizes in ((640, False, [(427, 640), (640, 480), (3000, 2000), (3300, 2200), (97, 131), (640, 640)]),
                            (128, False, [(31 + i, 17 + 2 * i) for i in range(70)]),
                            (256, True, [(300, 400), (150, 200), (600, 800)])):
        images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
        raw = torch.from_numpy(np.concatenate([im.ravel() for im in images])).to(dev)
        n = len(images)
        targets = [transforms.rescale_size(w, h, T, fixed) for h, w in sizes]
        up = lambda v: (v + 127) // 128 * 128  # noqa: E731
        PH, PW = (up(targets[0][1]), up(targets[0][0])) if fixed else (T, T)
        offs, hw4, ltrb = (C.c_long * n)(), (C.c_int * (4 * n))(), (C.c_int * (4 * n))()
        o = 0
        one = torch.empty((n, 3, PH, PW), device=dev)
        for i, (h, w) in enumerate(sizes):
            offs[i] = o
            hw4[4 * i:4 * i + 4] = [h, w, targets[i][1], targets[i][0]]
            l4 = (C.c_int * 4)()
            _lib.check(lib.og_rescale_pad_normalize_u8(C.c_void_p(raw.data_ptr() + o), h, w, targets[i][1], targets[i][0], PH, PW, int(fixed),
                                                       mean, std, fill, _lib.ptr(one[i]), l4, _lib.stream_ptr(dev)), lib)
            o += h * w * 3
            one_ltrb = list(l4) if i == 0 else one_ltrb + list(l4)
        got = torch.full((n, 3, PH, PW), float('nan'), device=dev)
        _lib.check(lib.og_rescale_pad_normalize_batch_u8(_lib.ptr(raw), offs, hw4, n, PH, PW, int(fixed), mean, std, fill, _lib.ptr(got),
                                                         ltrb, _lib.stream_ptr(dev)), lib)
        assert torch.equal(got, one) and list(ltrb) == one_ltrb, (T, fixed)
    hw_bad = (C.c_int * 4)(10, 10, 700, 700)
    rc = lib.og_rescale_pad_normalize_batch_u8(_lib.ptr(raw), (C.c_long * 1)(0), hw_bad, 1, 640, 640, 0, mean, std, fill, _lib.ptr(got), None,
                                               _lib.stream_ptr(dev))
    assert rc == _lib.OG_EINVAL and b'must fit the target' in lib.og_last_error()


def _mask_cases():
    rng = np.random.default_rng(5)
    m = np.full((3, 128, 192), 255, np.uint8)
    m[0, 20:60, 30:100] = 0                                   # a box
    yy, xx = np.mgrid[:128, :192]
    m[1][(yy - 64) ** 2 + (xx - 90) ** 2 < 40 ** 2] = 0      # a disc
    m[2] = (rng.random((128, 192)) > 0.3).astype(np.uint8) * 255   # salt and pepper: the cubic taps overshoot
    return m


def test_oracle_shrink_mask_miss():
    """ogo_shrink_mask_miss_u8 (encoder/heatmap.py:56-60): far from an edge the mask survives, the result is boolean at 1/4
    resolution and equals the restated resize + threshold."""
    import oracle
    m = _mask_cases()
    for i in range(3):
        out = oracle.shrink_mask_miss_u8(m[i], 4)
        assert out.shape == (32, 48) and out.dtype == bool
    box = oracle.shrink_mask_miss_u8(m[0], 4)
    assert box[:4].all() and not box[7:13, 9:23].any()
    # the one-channel resize agrees with the three-channel one the input chain uses
    rgb = np.repeat(m[2][:, :, None], 3, 2)
    assert np.array_equal(oracle.resize_cubic_u8(rgb, 32, 48)[:, :, 0].astype(np.float32) / 255 > 0.7, oracle.shrink_mask_miss_u8(m[2], 4))


@pytest.mark.gpu
def test_shrink_mask_miss_device_matches_oracle():
    import oracle
    from offsetguided_amd.encoder import factory as ef
    m = _mask_cases()
    got = ef._mask(m, 3, 32, 48, torch.device('cuda:0'), 4).cpu().numpy()[:, 0]
    for i in range(3):
        assert np.array_equal(got[i], oracle.shrink_mask_miss_u8(m[i], 4)), i
    passthrough = ef._mask(got[:, None], 3, 32, 48, torch.device('cuda:0'), 4)
    assert passthrough.dtype == torch.bool and np.array_equal(passthrough.cpu().numpy()[:, 0], got)
    with pytest.raises(ValueError):
        ef._mask(m[:, :100], 3, 32, 48, torch.device('cuda:0'), 4)


# ---- cv2-generated vectors (tools/gen_golden_cv2.py): present only once a machine with opencv-python has produced them ----
_CV2_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resize_cv2.npz')
needs_cv2_golden = pytest.mark.skipif(not os.path.exists(_CV2_GOLDEN),
                                      reason='tests/golden/resize_cv2.npz absent: no machine with cv2 has run tools/gen_golden_cv2.py '
                                             'yet (f2 / mask-shrink parity with OpenCV itself stays unpinned)')


def _cv2_cases():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_golden_cv2', os.path.join(os.path.dirname(_CV2_GOLDEN), '..', '..', 'tools',
                                                                                 'gen_golden_cv2.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, np.load(_CV2_GOLDEN)


def _check_against_cv2(resize, shrink):
    mod, g = _cv2_cases()
    for i, ((h, w), T) in enumerate(mod.SMALL):
        tw, th = mod.target(h, w, T)
        assert np.array_equal(resize(mod.image(200 + i, h, w), th, tw), g[f'small{i}']), ('small', i)
    for i, ((h, w), T) in enumerate(mod.CASES):
        tw, th = mod.target(h, w, T)
        r = resize(mod.image(100 + i, h, w), th, tw)
        assert np.array_equal(r[:48, :48], g[f'big{i}_corner']) and mod.sha(r) == str(g[f'big{i}_sha']), ('big', i)
    m = mod.masks()
    for i in range(3):
        assert np.array_equal(shrink(m, i), g['masks'][i]), ('mask', i)


@needs_cv2_golden
def test_oracle_resize_matches_cv2_vectors():
    """The oracle's restatement of cv2.resize(INTER_CUBIC) and of the mask shrink against OpenCV's own outputs."""
    import oracle
    _check_against_cv2(lambda im, th, tw: oracle.resize_cubic_u8(im, th, tw), lambda m, i: oracle.shrink_mask_miss_u8(m[i], 4))


@needs_cv2_golden
@pytest.mark.gpu
def test_device_resize_matches_cv2_vectors():
    """og_resize_cubic_u8 / og_shrink_mask_miss_u8 against OpenCV's own outputs."""
    from offsetguided_amd.encoder import factory as ef
    dev = torch.device('cuda:0')
    _check_against_cv2(lambda im, th, tw: transforms.resize_cubic(im, th, tw).cpu().numpy(),
                       lambda m, i: ef._mask(m, 3, 32, 48, dev, 4).cpu().numpy()[i, 0])
