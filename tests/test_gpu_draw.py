"""GPU: the pose painter (og_draw_poses_u8, csrc/draw.hip; visualization.draw_poses; evaluate.run_images --show-detected-poses).

Every kernel case asserts np.array_equal(kernel, draw_reference(..., np.float32)): the specification makes every operation one correctly
rounded fp32 operation in a fixed order, in the kernel and in the numpy restatement (tests/draw_common.py) alike, so equality is the
requirement and no tolerance applies.  The cases (draw_common.cases) are the smallest shapes at which the kernel can go wrong: partial
tiles, segments on tile and wave seams, masked inputs, more primitives over one tile than the LDS list holds, the parameter grid."""
import numpy as np
import pytest
import torch

from draw_common import CASES, LIST_CAP, TOY, reference
from offsetguided_amd import _lib, evaluate, models, visualization

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def paint(case, dev, as_list=False):
    images = torch.from_numpy(case['images'].copy()).to(dev)
    kw = dict(line_width=case['line_width'], marker_radius=case['marker_radius'], alpha=case['alpha'], palette=case['palette'])
    if as_list:
        poses = [case['poses'][n, :case['n_persons'][n]] for n in range(len(case['n_persons']))]
        out = visualization.draw_poses(images, poses, case['skeleton'], **kw)
    else:
        out = visualization.draw_poses(images, case['poses'], case['skeleton'], n_persons=case['n_persons'], **kw)
    assert out is images                                   # painted in place
    return images.cpu().numpy()


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_equals_the_fp32_restatement(dev, name):
    got, ref = paint(CASES[name], dev), reference(name)
    bad = np.argwhere((got != ref).any(axis=3))
    assert np.array_equal(got, ref), f'{len(bad)} pixels differ, first (n, row, col) {bad[:5].tolist()}'


def test_image_without_persons_comes_back_byte_identical(dev):
    case = CASES['masked']
    assert case['n_persons'][1] == 0
    got = paint(case, dev)
    assert np.array_equal(got[1], case['images'][1])
    assert (got[0] != case['images'][0]).any() and (got[2] != case['images'][2]).any()


@pytest.mark.parametrize('name', ['partial_tiles', 'masked'])
def test_list_of_per_image_arrays(dev, name):
    """The form PostProcess hands out: a list of (P_n, K, >= 3) arrays (an image without persons: an empty array), extra columns ignored."""
    case = dict(CASES[name])
    case['poses'] = np.concatenate([case['poses'], np.full(case['poses'].shape[:3] + (3,), 7.0, np.float32)], axis=3)
    assert np.array_equal(paint(case, dev, as_list=True), reference(name))


def test_overflow_case_exceeds_the_list(dev):
    """The overflow case really puts more primitives on one tile than the list holds: every primitive of it lies within tile (1, 0)'s
    grown box (columns 32 ... 63, rows 0 ... 7)."""
    case = CASES['overflow']
    xy = case['poses'][0, :, :, :2]
    assert (xy[..., 0] >= 32).all() and (xy[..., 0] <= 63).all() and (xy[..., 1] >= 0).all() and (xy[..., 1] <= 7).all()
    vis = case['poses'][0, :, :, 2] > 0
    n_prims = sum(int(v[a] and v[b]) for v in vis for a, b in TOY) + int(vis.sum())
    assert n_prims == LIST_CAP + 70


def test_errors(dev):
    lib = _lib.load()
    case = CASES['partial_tiles']
    with pytest.raises(_lib.OgError):                                         # a CPU tensor
        visualization.draw_poses(torch.from_numpy(case['images'].copy()), case['poses'], case['skeleton'], n_persons=case['n_persons'])
    images = torch.from_numpy(case['images'].copy()).to(dev)
    with pytest.raises(ValueError):                                           # a skeleton index beyond K: raised on the host
        visualization.draw_poses(images, case['poses'], [(0, 1), (2, 18)], n_persons=case['n_persons'])
    with pytest.raises(ValueError):
        visualization.draw_poses(images, case['poses'], case['skeleton'], n_persons=[3, 4])      # more persons than rows
    with pytest.raises(_lib.OgError, match='alpha'):
        visualization.draw_poses(images, case['poses'], case['skeleton'], n_persons=case['n_persons'], alpha=0.0)
    # the C entry itself: OG_EINVAL and a message, nothing launched
    poses = torch.from_numpy(case['poses']).to(dev)
    counts = torch.tensor(case['n_persons'], dtype=torch.int32, device=dev)
    skel = torch.tensor(case['skeleton'], dtype=torch.int32, device=dev)
    pal = torch.from_numpy(visualization.TAB20.copy()).to(dev)
    N, H, W, _ = images.shape

    def call(n_colors=20, alpha=1.0, H=H):
        return lib.og_draw_poses_u8(_lib.ptr(images), _lib.ptr(poses), _lib.ptr(counts), _lib.ptr(skel), _lib.ptr(pal), n_colors, N, H, W,
                                    3, 17, 19, 2.0, 3.0, alpha, _lib.stream_ptr(dev))
    assert call(alpha=0.0) == _lib.OG_EINVAL and b'alpha' in lib.og_last_error()
    assert call(alpha=1.5) == _lib.OG_EINVAL and b'alpha' in lib.og_last_error()
    assert call(n_colors=0) == _lib.OG_EINVAL and b'n_colors' in lib.og_last_error()
    assert call(H=0) == _lib.OG_EINVAL and b'bad shape' in lib.og_last_error()
    torch.cuda.synchronize(dev)
    assert np.array_equal(images.cpu().numpy(), case['images'])               # none of the refused calls painted anything
    assert call() == _lib.OG_OK
    assert np.array_equal(images.cpu().numpy(), reference('partial_tiles'))


def test_denormalise_u8_recovers_the_pixels(dev):
    """The network-input batch (v / 255 - mean) / std, as the input chain writes it, goes back to the uint8 pixels v exactly."""
    from offsetguided_amd.config import data_mean, data_std
    v = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (2, 3, 16, 24), dtype=np.uint8)).to(dev)
    mean = torch.tensor(data_mean, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(data_std, device=dev).view(1, 3, 1, 1)
    x = (v.float() / 255.0 - mean) / std
    assert torch.equal(visualization.denormalise_u8(x), v.permute(0, 2, 3, 1))


def _read_ppm(path):
    raw = open(path, 'rb').read()
    magic, w, h, maxval = raw.split(maxsplit=4)[:4]
    assert magic == b'P6' and maxval == b'255'
    n = int(w) * int(h) * 3
    assert len(raw) == len(b'P6\n%d %d\n255\n' % (int(w), int(h))) + n
    return np.frombuffer(raw[len(raw) - n:], np.uint8).reshape(int(h), int(w), 3)


def test_run_images_writes_the_painted_batches(dev, tmp_path):
    """Two synthetic bs2 128x128 batches (tensor batches: painted on a black canvas): one P6 file per batch, recorded in
    stats['pose_images']; the returned keypoints are those of the same call without the flag."""
    torch.manual_seed(0)
    argv = ['--no-pretrain', '--initialize-whole', 'False', '--topk', '32', '--thre-hmp', '0.04', '--person-thre', '0.04', '--dist-max',
            '40', '--long-edge', '128', '--batch-size', '2', '--print-freq', '1000000', '--dump-name', 'run']
    model, _ = models.model_factory(evaluate.evaluate_cli(argv))
    plain_stats = {}
    plain, plain_ids = evaluate.run_images(evaluate.evaluate_cli(argv), model=model, n_synthetic_batches=2, stats=plain_stats)
    assert 'pose_images' not in plain_stats and not list(tmp_path.iterdir())
    stats = {}
    shown, ids = evaluate.run_images(evaluate.evaluate_cli(argv + ['--show-detected-poses', '--show-dir', str(tmp_path / 'shown')]),
                                     model=model, n_synthetic_batches=2, stats=stats)
    assert ids == plain_ids == [0, 1, 2, 3] and shown == plain
    assert stats['pose_images'] == [str(tmp_path / 'shown' / f'run.poses.{b}.ppm') for b in (0, 1)]
    for b, path in enumerate(stats['pose_images']):
        img = _read_ppm(path)
        assert img.shape == (128, 128, 3)
        detected = any(r['image_id'] == 2 * b and r['score'] != 0.01 for r in shown)     # the first image of batch b
        assert bool(img.any()) == detected, 'a black canvas is painted exactly where somebody was detected'
