"""GPU: the model-inspection views (csrc/views.hip: og_draw_heatmap_u8, og_draw_segments_u8, og_limbs_to_segments_f32,
og_offsets_to_segments_f32; visualization.draw_heatmap / draw_segments / draw_limbs / draw_offsets; evaluate.run_images --show-hmp-idx /
--show-all-limbs / --show-limb-idx).

Every kernel case asserts equality with the fp32 numpy restatement of the header's specification (tests/views_common.py): every
operation is one correctly rounded fp32 operation in a fixed order on both sides, so no tolerance applies.  The cases are the smallest
shapes at which each kernel can go wrong (views_common.*_cases)."""
import numpy as np
import pytest
import torch

import views_common as vc
from offsetguided_amd import _lib, decoder, evaluate, models, transforms, visualization
from offsetguided_amd.config import coco_data as cd

pytestmark = pytest.mark.gpu
SENTINEL = -77.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def _differ(got, ref):
    bad = np.argwhere((got != ref).any(axis=-1))
    return f'{len(bad)} pixels differ, first (n, row, col) {bad[:5].tolist()}'


# ------------------------------------------------------------------------------------------------------------ heat-map overlay
@pytest.mark.parametrize('name', sorted(vc.HEATMAP_CASES))
def test_heatmap_equals_the_fp32_restatement(dev, name):
    c = vc.HEATMAP_CASES[name]
    images = torch.from_numpy(c['images'].copy()).to(dev)
    out = visualization.draw_heatmap(images, torch.from_numpy(c['hm']).to(dev), c['channel'], nms=bool(c['nms']), vmin=c['vmin'],
                                     vmax=c['vmax'], alpha=c['alpha'], colormap=c['lut'])
    assert out is images
    got, ref = images.cpu().numpy(), vc.heatmap_expected(name)
    assert np.array_equal(got, ref), _differ(got, ref)


def test_heatmap_values_are_those_of_the_upsample_kernel(dev):
    """The restatement's input, the oracle's x4 plane, is what og_upsample_bicubic4_f32 writes."""
    for name in ('multi_nms1', 'peaks'):
        c = vc.HEATMAP_CASES[name]
        up = decoder.factory.upsample4(torch.from_numpy(c['hm']).to(dev), 'bicubic')[:, c['channel']].cpu().numpy()
        assert np.array_equal(up, vc.hires(c))


# ------------------------------------------------------------------------------------------------------------- segment painter
def _paint_segments(c, dev):
    images = torch.from_numpy(c['images'].copy()).to(dev)
    out = visualization.draw_segments(images, torch.from_numpy(c['segs']).to(dev), torch.tensor(c['n_segs'], dtype=torch.int32, device=dev),
                                      line_color=c['line_rgb'], marker_color=c['marker_rgb'], line_width=c['line_width'],
                                      start_radius=c['r_start'], end_radius=c['r_end'], alpha=c['alpha'])
    assert out is images
    return images.cpu().numpy()


@pytest.mark.parametrize('name', sorted(vc.SEGMENT_CASES))
def test_segments_equal_the_fp32_restatement(dev, name):
    got, ref = _paint_segments(vc.SEGMENT_CASES[name], dev), vc.segments_expected(name)
    assert np.array_equal(got, ref), _differ(got, ref)


def test_segment_order_is_part_of_the_result(dev):
    ab, ba = _paint_segments(vc.SEGMENT_CASES['order_ab'], dev), _paint_segments(vc.SEGMENT_CASES['order_ba'], dev)
    assert (ab != ba).any()
    assert np.array_equal(ab, vc.segments_expected('order_ab')) and np.array_equal(ba, vc.segments_expected('order_ba'))


def test_segments_without_counts_paint_every_row(dev):
    c = dict(vc.SEGMENT_CASES['order_ab'])
    images = torch.from_numpy(c['images'].copy()).to(dev)
    visualization.draw_segments(images, torch.from_numpy(c['segs']).to(dev), line_width=c['line_width'])
    assert np.array_equal(images.cpu().numpy(), vc.segments_expected('order_ab'))


# ----------------------------------------------------------------------------------------------------------------- compactions
def _check_compaction(segs, n_segs, expected):
    segs, n_segs = segs.cpu().numpy(), n_segs.cpu().numpy()
    assert n_segs.tolist() == [len(e) for e in expected]
    for n, e in enumerate(expected):
        assert np.array_equal(segs[n, :len(e)], e), f'image {n}: kept rows differ'
        assert (segs[n, len(e):] == SENTINEL).all(), f'image {n}: rows past the count were written'


@pytest.mark.parametrize('name', sorted(vc.LIMB_TABLES))
def test_limbs_to_segments(dev, name):
    c = vc.LIMB_TABLES[name]
    lib = _lib.load()
    limbs = torch.from_numpy(c['limbs']).to(dev)
    N, L, K, _ = limbs.shape
    segs = torch.full((N, L * K, 4), SENTINEL, dtype=torch.float32, device=dev)
    n_segs = torch.full((N,), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.og_limbs_to_segments_f32(_lib.ptr(limbs), N, L, K, -1 if c['limb'] is None else c['limb'], c['dist_max'], _lib.ptr(segs),
                                            _lib.ptr(n_segs), _lib.stream_ptr(dev)), lib)
    _check_compaction(segs, n_segs, vc.limbs_expected(name))
    # the wrapper: the same rows and counts
    w_segs, w_n = visualization.limbs_to_segments(limbs, limb=c['limb'], dist_max=c['dist_max'])
    assert torch.equal(w_n, n_segs) and all(torch.equal(w_segs[n, :int(k)], segs[n, :int(k)]) for n, k in enumerate(n_segs.tolist()))


@pytest.mark.parametrize('name', sorted(vc.OFFSET_FIELDS))
def test_offsets_to_segments(dev, name):
    c = vc.OFFSET_FIELDS[name]
    lib = _lib.load()
    hm, off = torch.from_numpy(c['hm']).to(dev), torch.from_numpy(c['off']).to(dev)
    N, C, h, w = hm.shape
    S = lib.og_offsets_segments_capacity(h, w, c['step'])
    assert S == -(-4 * h // c['step']) * -(-4 * w // c['step'])
    segs = torch.full((N, S, 4), SENTINEL, dtype=torch.float32, device=dev)
    n_segs = torch.full((N,), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.og_offsets_to_segments_f32(_lib.ptr(hm), _lib.ptr(off), N, C, off.shape[1] // 2, h, w, c['joint_from'], c['limb'],
                                              c['step'], c['thre'], _lib.ptr(segs), _lib.ptr(n_segs), _lib.stream_ptr(dev)), lib)
    _check_compaction(segs, n_segs, vc.offsets_expected(name))


def test_offset_planes_are_those_of_the_upsample_kernels(dev):
    c = vc.OFFSET_FIELDS['step1']
    heat, U, V = vc.offset_planes(c)
    up = decoder.factory.upsample4(torch.from_numpy(c['off']).to(dev), 'bilinear').cpu().numpy()
    assert np.array_equal(up[:, 2 * c['limb']], U, equal_nan=True) and np.array_equal(up[:, 2 * c['limb'] + 1], V, equal_nan=True)
    assert np.array_equal(decoder.factory.upsample4(torch.from_numpy(c['hm']).to(dev), 'bicubic').cpu().numpy()[:, c['joint_from']], heat)


def test_draw_limbs_and_draw_offsets_are_compaction_then_painter(dev):
    c = vc.LIMB_TABLES['random']
    base = vc._base(2, 64, 64, 9)
    images = torch.from_numpy(base.copy()).to(dev)
    assert visualization.draw_limbs(images, torch.from_numpy(c['limbs']).to(dev), dist_max=c['dist_max'], alpha=0.5) is images
    exp = vc.limbs_expected('random')
    table = np.zeros((2, max(len(e) for e in exp), 4), np.float32)
    for n, e in enumerate(exp):
        table[n, :len(e)] = e
    ref = vc.segments_reference(base, table, [len(e) for e in exp], (255, 0, 0), (0, 128, 0), 2.0, 3.0, 3.0, 0.5, np.float32)
    assert np.array_equal(images.cpu().numpy(), ref)
    c = vc.OFFSET_FIELDS['step3']
    skeleton = [(2, 0), (0, 1), (1, 2), (2, 1)]
    base = vc._base(2, 20, 44, 10)
    images = torch.from_numpy(base.copy()).to(dev)
    out = visualization.draw_offsets(images, torch.from_numpy(c['hm']).to(dev), torch.from_numpy(c['off']).to(dev), c['limb'], skeleton,
                                     step=c['step'], thre=c['thre'])
    assert out is images and skeleton[c['limb']][0] == c['joint_from']
    exp = vc.offsets_expected('step3')
    table = np.zeros((2, max(len(e) for e in exp), 4), np.float32)
    for n, e in enumerate(exp):
        table[n, :len(e)] = e
    ref = vc.segments_reference(base, table, [len(e) for e in exp], (255, 0, 0), (0, 128, 0), 2.0, 0.0, 1.5, 1.0, np.float32)
    assert np.array_equal(images.cpu().numpy(), ref)


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_every_documented_einval_leaves_the_image_untouched(dev):
    lib = _lib.load()
    E = _lib.OG_EINVAL
    st = _lib.stream_ptr(dev)
    inf, nan = float('inf'), float('nan')
    images = torch.full((2, 20, 44, 3), 99, dtype=torch.uint8, device=dev)
    hm = torch.rand(2, 3, 5, 11, device=dev)
    off = torch.rand(2, 8, 5, 11, device=dev)
    lut = torch.from_numpy(visualization.VIRIDIS.copy()).to(dev)
    P = _lib.ptr

    def heat(images=P(images), hm=P(hm), lut=P(lut), n_colors=256, N=2, C=3, h=5, w=11, channel=0, vmin=0.0, vmax=1.0, alpha=0.8, nms=1):
        return lib.og_draw_heatmap_u8(images, hm, lut, n_colors, N, C, h, w, channel, vmin, vmax, alpha, nms, st)
    for kw in (dict(images=None), dict(hm=None), dict(lut=None), dict(N=0), dict(C=0), dict(h=0), dict(w=-1), dict(h=2 ** 30),
               dict(channel=-1), dict(channel=3), dict(n_colors=0), dict(vmin=nan), dict(vmax=inf), dict(vmin=-inf), dict(vmax=0.0),
               dict(vmin=1.0, vmax=0.5), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=nan), dict(N=65536), dict(h=4 * 65536)):
        assert heat(**kw) == E and b'og_draw_heatmap_u8' in lib.og_last_error(), kw
    segs = torch.rand(2, 8, 4, device=dev) * 20
    n_segs = torch.full((2,), 8, dtype=torch.int32, device=dev)

    def paint(images=P(images), segs=P(segs), n_segs=P(n_segs), N=2, H=20, W=44, S=8, lw=2.0, rs=3.0, re=3.0, alpha=1.0):
        return lib.og_draw_segments_u8(images, segs, n_segs, N, H, W, S, 255, 255 << 8, lw, rs, re, alpha, st)
    for kw in (dict(images=None), dict(segs=None), dict(n_segs=None), dict(N=0), dict(H=0), dict(W=0), dict(S=0), dict(alpha=0.0),
               dict(alpha=2.0), dict(lw=-1.0), dict(lw=inf), dict(rs=-0.5), dict(rs=nan), dict(re=-1.0), dict(re=inf),
               dict(segs=segs.data_ptr() + 4), dict(S=2 ** 29), dict(N=65536), dict(H=8 * 65536)):
        assert paint(**kw) == E and b'og_draw_segments_u8' in lib.og_last_error(), kw
    limbs = torch.rand(2, 4, 3, 13, device=dev)
    out = torch.full((2, 12, 4), SENTINEL, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int32, device=dev)

    def compact(limbs=P(limbs), N=2, L=4, K=3, limb=-1, segs=P(out), n_segs=P(counts)):
        return lib.og_limbs_to_segments_f32(limbs, N, L, K, limb, 20.0, segs, n_segs, st)
    for kw in (dict(limbs=None), dict(segs=None), dict(n_segs=None), dict(N=0), dict(L=0), dict(K=0), dict(L=2 ** 20, K=2 ** 10), dict(limb=4),
               dict(segs=out.data_ptr() + 4)):
        assert compact(**kw) == E and b'og_limbs_to_segments_f32' in lib.og_last_error(), kw
    grid = torch.full((2, 880, 4), SENTINEL, device=dev)

    def arrows(hm=P(hm), off=P(off), N=2, C=3, L=4, h=5, w=11, joint_from=0, limb=0, step=7, segs=P(grid), n_segs=P(counts)):
        return lib.og_offsets_to_segments_f32(hm, off, N, C, L, h, w, joint_from, limb, step, 0.2, segs, n_segs, st)
    for kw in (dict(hm=None), dict(off=None), dict(segs=None), dict(n_segs=None), dict(N=0), dict(C=0), dict(L=0), dict(h=0), dict(w=0),
               dict(h=2 ** 22 + 1), dict(joint_from=-1), dict(joint_from=3), dict(limb=-1), dict(limb=4), dict(step=0), dict(step=-7),
               dict(segs=grid.data_ptr() + 8), dict(h=2 ** 14, w=2 ** 14, step=1)):
        assert arrows(**kw) == E and b'og_offsets_to_segments_f32' in lib.og_last_error(), kw
    assert lib.og_offsets_segments_capacity(0, 11, 7) == 0 and lib.og_offsets_segments_capacity(5, 11, 0) == 0
    torch.cuda.synchronize(dev)
    assert bool((images == 99).all()) and bool((out == SENTINEL).all()) and bool((grid == SENTINEL).all()) and bool((counts == -1).all())
    assert heat() == _lib.OG_OK and paint() == _lib.OG_OK and compact() == _lib.OG_OK and arrows() == _lib.OG_OK
    torch.cuda.synchronize(dev)
    assert not bool((images == 99).all()) and bool((counts >= 0).all())


def test_python_wrappers_refuse_before_anything_launches(dev):
    c = vc.HEATMAP_CASES['multi_nms0']
    base = torch.from_numpy(c['images'].copy())
    images, hm = base.to(dev), torch.from_numpy(c['hm']).to(dev)
    off = torch.zeros(2, 8, 9, 35, device=dev)
    segs = torch.zeros(2, 3, 4, device=dev)
    skeleton = [(0, 1), (1, 2), (2, 0), (0, 2)]
    V = visualization
    for call in (lambda: V.draw_heatmap(base, hm, 0), lambda: V.draw_heatmap(images, hm.cpu(), 0),       # host tensors
                 lambda: V.draw_segments(base, segs), lambda: V.draw_segments(images, segs.cpu()),
                 lambda: V.draw_segments(images, segs, torch.zeros(2, dtype=torch.int32)),
                 lambda: V.draw_limbs(images, torch.zeros(2, 4, 3, 13)), lambda: V.draw_limbs(base, torch.zeros(2, 4, 3, 13, device=dev)),
                 lambda: V.draw_offsets(images, hm.cpu(), off, 0, skeleton), lambda: V.draw_offsets(images, hm, off.cpu(), 0, skeleton),
                 lambda: V.draw_offsets(base, hm, off, 0, skeleton)):
        with pytest.raises(_lib.OgError):
            call()
    for call in (lambda: V.draw_heatmap(images.float(), hm, 0), lambda: V.draw_heatmap(images[:, :, :, :2], hm, 0),   # dtypes and shapes
                 lambda: V.draw_heatmap(images, hm.double(), 0), lambda: V.draw_heatmap(images, hm[:, :, :8], 0),
                 lambda: V.draw_heatmap(images, hm[:1], 0), lambda: V.draw_heatmap(images, hm, 3), lambda: V.draw_heatmap(images, hm, -1),
                 lambda: V.draw_heatmap(images, hm, 0, vmin=1.0, vmax=1.0), lambda: V.draw_heatmap(images, hm, 0, vmax=float('inf')),
                 lambda: V.draw_heatmap(images, hm, 0, colormap=np.zeros((4, 3), np.float32)),
                 lambda: V.draw_heatmap(images, hm, 0, colormap=np.zeros((0, 3), np.uint8)),
                 lambda: V.draw_segments(images, segs.double()), lambda: V.draw_segments(images, segs[:, :, :3]),
                 lambda: V.draw_segments(images, segs[:1]), lambda: V.draw_segments(images, segs, torch.zeros(2, dtype=torch.int64, device=dev)),
                 lambda: V.draw_segments(images, segs, torch.zeros(3, dtype=torch.int32, device=dev)),
                 lambda: V.draw_segments(images, segs, line_color=(256, 0, 0)), lambda: V.draw_segments(images, segs, marker_color=(1, 2)),
                 lambda: V.draw_limbs(images, torch.zeros(2, 4, 3, 12, device=dev)), lambda: V.draw_limbs(images, torch.zeros(1, 4, 3, 13, device=dev)),
                 lambda: V.draw_limbs(images, torch.zeros(2, 4, 3, 13, device=dev), limb=4),
                 lambda: V.draw_limbs(images, torch.zeros(2, 4, 3, 13, dtype=torch.float64, device=dev)),
                 lambda: V.draw_offsets(images, hm, off[:, :6], 0, skeleton), lambda: V.draw_offsets(images, hm, off, 4, skeleton),
                 lambda: V.draw_offsets(images, hm, off, 0, [(3, 1), (1, 2), (2, 0), (0, 2)]),
                 lambda: V.draw_offsets(images, hm, off, 0, skeleton, step=0), lambda: V.draw_offsets(images, hm, off.double(), 0, skeleton)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.OgError, match='alpha'):
        V.draw_heatmap(images, hm, 0, alpha=0.0)
    with pytest.raises(_lib.OgError, match='alpha'):
        V.draw_segments(images, segs, alpha=1.5)
    torch.cuda.synchronize(dev)
    assert torch.equal(images.cpu(), base)                     # nothing was painted by any refused call


# ------------------------------------------------------------------------------------------------------------------ end to end
def _read_ppm(path):
    raw = open(path, 'rb').read()
    magic, w, h, maxval = raw.split(maxsplit=4)[:4]
    assert magic == b'P6' and maxval == b'255'
    n = int(w) * int(h) * 3
    assert len(raw) == len(b'P6\n%d %d\n255\n' % (int(w), int(h))) + n
    return np.frombuffer(raw[len(raw) - n:], np.uint8).reshape(int(h), int(w), 3)


ARGV = ['--no-pretrain', '--initialize-whole', 'False', '--topk', '32', '--thre-hmp', '0.04', '--person-thre', '0.04', '--dist-max', '40',
        '--long-edge', '128', '--batch-size', '2', '--print-freq', '1000000', '--dump-name', 'run']


def _raw_loader():
    rng = np.random.default_rng(12)
    raw = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(100, 128), (128, 90), (64, 120), (128, 128)]]
    return [(raw[0:2], [None] * 2, [{'image_id': 1}, {'image_id': 2}]), (raw[2:4], [None] * 2, [{'image_id': 3}, {'image_id': 4}])]


@pytest.mark.parametrize('flip', [False, True])
def test_run_images_writes_the_views(dev, tmp_path, monkeypatch, flip):
    """Two bs2 batches of raw uint8 images at long edge 128: four files per batch, and batch 0's limbs view is draw_limbs applied by hand
    to generate_limbs of the outputs the harness submitted; with the flags off nothing is written and the results are the same."""
    torch.manual_seed(0)
    extra = ['--flip-test'] if flip else []
    model, _ = models.model_factory(evaluate.evaluate_cli(ARGV))
    plain_stats = {}
    plain, plain_ids = evaluate.run_images(evaluate.evaluate_cli(ARGV + extra), data_loader=_raw_loader(), model=model, stats=plain_stats)
    assert 'view_images' not in plain_stats and not list(tmp_path.iterdir())
    submitted = []
    real = decoder.PostProcess.submit

    def spy(self, features, **kw):
        submitted.append(([t.clone() for t in (features[self.hmp_index][0][self.feat_stage], features[self.omp_index][0][self.feat_stage])], kw))
        return real(self, features, **kw)
    monkeypatch.setattr(decoder.PostProcess, 'submit', spy)
    args = evaluate.evaluate_cli(ARGV + extra + ['--show-hmp-idx', '3', '--show-limb-idx', '5', '--show-all-limbs', '--show-dir',
                                                 str(tmp_path / 'views')])
    stats = {}
    shown, ids = evaluate.run_images(args, data_loader=_raw_loader(), model=model, stats=stats)
    assert ids == plain_ids == [1, 2, 3, 4] and shown == plain
    names = ['hmp3', 'hmp3_nms', 'limbs', 'limb5']
    assert stats['view_images'] == [str(tmp_path / 'views' / f'run.{name}.{b}.ppm') for b in (0, 1) for name in names]
    views = {(name, b): _read_ppm(str(tmp_path / 'views' / f'run.{name}.{b}.ppm')) for b in (0, 1) for name in names}
    assert all(v.shape == (128, 128, 3) for v in views.values())
    # by hand, batch 0: the canvas is the network-input image, the limbs those of the submitted outputs
    (hm, off), kw = submitted[0]
    assert kw['flip_test'] == flip and tuple(hm.shape) == (4 if flip else 2, 17, 32, 32)
    x, _ = transforms.EvalPreprocess(128, device=dev)(list(_raw_loader()[0][0]), image_ids=[1, 2])
    canvas = visualization.denormalise_u8(x[:1])
    proc = decoder.decoder_factory(args)
    feats = [([hm], [[]], [[]]), ([off], [[]], [[]])]
    limbs = proc.generate_limbs(feats, flip_test=flip)
    by_hand = visualization.draw_limbs(canvas.clone(), limbs[:1], dist_max=40.0)
    assert np.array_equal(views[('limbs', 0)], by_hand[0].cpu().numpy())
    # and the heat-map views are draw_heatmap on the decoded maps
    d_hm, d_off = evaluate.decoded_maps(proc, feats, flip)
    assert tuple(d_hm.shape) == (2, 17, 32, 32) and tuple(d_off.shape) == (2, 38, 32, 32)
    for name, nms in (('hmp3', False), ('hmp3_nms', True)):
        assert np.array_equal(views[(name, 0)], visualization.draw_heatmap(canvas.clone(), d_hm[:1], 3, nms=nms)[0].cpu().numpy())
    faded = (canvas >> 1) + 128
    arrows = visualization.draw_offsets(faded, d_hm[:1], d_off[:1], 5, cd.COCO_PERSON_SKELETON)
    assert np.array_equal(views[('limb5', 0)], arrows[0].cpu().numpy())
    assert (views[('hmp3', 0)] != canvas[0].cpu().numpy()).any()
