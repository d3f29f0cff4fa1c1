"""CPU: the host side of the photometric augmentation (offsetguided_amd/transforms/photometric.py) against the fixture generated from
the imported reference (tests/golden/augment_photometric.npz, tools/gen_golden_photometric.py), and the numpy restatement of the
device specification (tests/photometric_common.py) against the oracles this machine has: PIL's `L` conversion, PIL's quantisation
tables and PIL's JPEG round trip."""
import io
import json
import os
import random
import re

import numpy as np
import pytest

import photometric_common as pc
from offsetguided_amd import _lib, transforms as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('og_warp_affine_photo_batch_u8', 'og_jpeg_roundtrip_batch_u8', 'og_affine_joints_jitter_f32')


@pytest.fixture(scope='module')
def gold():
    z = np.load(pc.GOLDEN)
    return {k: z[k] for k in z.files}


def test_fixture_covers_what_it_should(gold):
    assert len(gold['gate']) == 64 and set(gold['prob'].tolist()) == {0.2, 0.5, 0.9}
    assert 8 < gold['gate'].sum() < 56
    d = gold['deltas'][gold['gate']]
    assert (np.abs(d) <= [10, 40, 30]).all() and (d.min(axis=0) < [-5, -20, -15]).all() and (d.max(axis=0) > [5, 20, 15]).all()
    assert (gold['deltas'][~gold['gate']] == 0).all()
    assert {tuple(g) for g in gold['chain_gates'].tolist()} == {(False, False), (False, True), (True, False), (True, True)}


def test_draw_classes_reproduce_the_reference(gold):
    """RandomApply's gate from `random`, ColorTint's three deltas from numpy.random: the same outcomes under the same seeds."""
    for c in range(64):
        random.seed(c)
        np.random.seed(c)
        drawn = T.RandomApply(T.ColorTint(), float(gold['prob'][c])).draw()
        assert (drawn is not None) == bool(gold['gate'][c]), c
        if drawn is not None:
            assert list(drawn) == gold['deltas'][c].tolist() and all(isinstance(v, int) for v in drawn), c


def test_draw_order_is_the_reference_chain(gold):
    """jpeg's gate before tint's, the deltas right behind tint's gate (draw_photo, as DeviceAugment calls it); explicit generators."""
    params = T.PhotoParams(tint_prob=0.5, jpeg_prob=0.5)
    for c in range(64):
        (d,) = T.draw_photo(params, [2], 17, random.Random(c), np.random.RandomState(c))
        assert [d['jpeg'] is not None, d['tint'] is not None] == gold['chain_gates'][c].tolist(), c
        assert d['jpeg'] in (None, 50) and d['gray'] is None and d['jitter'] is None
        if d['tint'] is not None:
            assert list(d['tint']) == gold['chain_deltas'][c].tolist(), c


def test_probability_zero_draws_nothing():
    """With the defaults the random stream stays untouched; each step draws its gate only when its probability is > 0."""
    rng = random.Random(5)
    state = rng.getstate()
    assert T.PhotoParams().steps() == []
    assert T.draw_photo(T.PhotoParams(), [1, 2], 17, rng) == [{'jitter': None, 'jpeg': None, 'tint': None, 'gray': None}] * 2
    assert rng.getstate() == state
    for kw, name in (({'jitter_prob': 1}, 'jitter'), ({'jpeg_prob': 1}, 'jpeg'), ({'tint_prob': 1}, 'tint'), ({'gray_prob': 1}, 'gray')):
        rng, twin = random.Random(5), random.Random(5)
        (d,) = T.draw_photo(T.PhotoParams(**kw), [3], 17, rng, np.random.RandomState(0))
        assert [k for k, v in d.items() if v is not None] == [name]
        twin.uniform(0, 1)
        assert rng.getstate() == twin.getstate()                       # exactly one gate
    (d,) = T.draw_photo(T.PhotoParams(jitter_prob=1), [3], 17, random.Random(0))
    assert d['jitter'].shape == (3, 17, 2) and d['jitter'].dtype == np.float32 and 0 <= d['jitter'].min() and d['jitter'].max() < 1
    p = T.PhotoParams()
    assert (p.jpeg_quality, p.jitter_epsilon, p.jitter_shift) == (50, 0.5, 0)
    assert (T.AnnotationJitter().shift, T.AnnotationJitter().epsilon, T.JpegCompression().quality) == (0, 0.5, 50)


def test_jitter_noise_is_torch_rand_per_person():
    import torch
    torch.manual_seed(3)
    got = T.AnnotationJitter().draw(persons=2, keypoints=17)
    torch.manual_seed(3)
    assert np.array_equal(got, np.stack([torch.rand(17, 2).numpy(), torch.rand(17, 2).numpy()]))


def test_photo_table():
    photo = [{'jitter': None, 'jpeg': None, 'tint': None, 'gray': None}, {'jitter': None, 'jpeg': 50, 'tint': (-3, 7, 30), 'gray': None},
             {'jitter': None, 'jpeg': None, 'tint': (1, 2, 3), 'gray': True}, {'jitter': None, 'jpeg': None, 'tint': None, 'gray': True}]
    table = T.photo_table(photo)
    assert table.dtype == np.int32 and table.tolist() == [[0, 0, 0, 0], [1, -3, 7, 30], [3, 1, 2, 3], [2, 0, 0, 0]]
    assert (pc.MODE_TINT, pc.MODE_GRAY) == (T.photometric.MODE_TINT, T.photometric.MODE_GRAY)


def test_gray_equals_pil():
    Image = pytest.importorskip('PIL.Image')
    lat = pc.lattice()
    assert len(lat) == 17 ** 3 + 256
    ours = pc.gray(lat[None])[0]
    pil = np.asarray(Image.fromarray(lat[None]).convert('L'))[0]
    assert np.array_equal(ours[:, 0], pil) and np.array_equal(ours[:, 1], pil) and np.array_equal(ours[:, 2], pil)


def test_division_tables():
    """The integer derivation equals rint of the quotient (no ties), as the header says."""
    i = np.arange(1, 256)
    assert np.array_equal(pc.SDIV[1:], np.rint((255 << 12) / i).astype(np.int64)) and pc.SDIV[0] == 0
    assert np.array_equal(pc.HDIV[1:], np.rint((180 << 12) / (6 * i)).astype(np.int64)) and pc.HDIV[0] == 0
    assert 5 * 255 * int(pc.HDIV.max()) + (1 << 11) < 2 ** 31 and 255 * int(pc.SDIV.max()) + (1 << 11) < 2 ** 31


def test_zero_tint_stays_within_the_derived_bound():
    """csrc/photometric.h: the largest channel exact, the smallest within 1, the middle one within 6 (TINT_BOUND)."""
    lat = pc.lattice()
    out = pc.tint(lat, 0, 0, 0).astype(np.int64)
    src = lat.astype(np.int64)
    assert np.abs(out - src).max() <= pc.TINT_BOUND == 6
    assert np.array_equal(out.max(axis=1), src.max(axis=1))
    assert np.abs(out.min(axis=1) - src.min(axis=1)).max() <= 1
    greys = lat[17 ** 3:]
    assert np.array_equal(pc.tint(greys, 7, 0, 0), greys)              # no saturation: the hue does not matter
    h, s, v = pc.rgb_to_hsv(lat)
    assert h.min() >= 0 and h.max() < 180 and s.min() >= 0 and s.max() == 255


def test_tint_clamps_and_does_not_wrap():
    red = np.array([[200, 10, 10]], np.uint8)                          # H = 0
    h, s, v = pc.rgb_to_hsv(red)
    assert (int(h[0]), int(v[0])) == (0, 200)
    assert np.array_equal(pc.tint(red, -10, 0, 0), pc.tint(red, 0, 0, 0))      # hue 0 - 10 clamps to 0, it does not become 170
    assert pc.tint(red, 0, 0, 100).max() == 255 and pc.tint(red, 0, 0, -250).max() == 0
    out = pc.tint(red, 0, -255, 0)
    assert (out == out[0, 0]).all()                                    # saturation 0: grey


def test_quant_tables_equal_pil():
    Image = pytest.importorskip('PIL.Image')
    for quality in (10, 50, 90):
        f = io.BytesIO()
        Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(f, 'jpeg', quality=quality)
        q = Image.open(f).quantization
        ours = pc.quant_tables(quality)
        assert list(q[0]) == ours[0].tolist() and list(q[1]) == ours[1].tolist(), quality
    assert pc.quant_tables(100)[0].tolist() == [1] * 64 and pc.quant_tables(1)[1].max() == 255


def test_dct_table_and_overflow_bounds():
    """The integer cosine table is the rounded orthonormal DCT matrix; the bounds of csrc/jpeg_sim.hip recomputed from it."""
    u, x = np.mgrid[0:8, 0:8]
    exact = np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    assert np.array_equal(pc.DCT, np.rint(exact * 8192).astype(np.int64))
    row, col = int(np.abs(pc.DCT).sum(axis=1).max()), int(np.abs(pc.DCT).sum(axis=0).max())
    assert (row, col) == (23168, 21641)
    t1 = (128 * row + 512) >> 10
    F = (t1 * row + (1 << 15)) >> 16
    t2 = ((F + 127) * row + 512) >> 10
    assert (t1, F, F + 127, t2) == (2896, 1024, 1151, 26041) and t2 * row + (1 << 15) == 603350656 < 2 ** 31


def test_jpeg_roundtrip_properties():
    flat = np.full((50, 50, 3), 128, np.uint8)
    assert np.array_equal(pc.jpeg_roundtrip(flat, 10), flat)                       # a flat grey block survives any quality
    rs = np.random.RandomState(0)
    im = pc.structured_images()[0][:50, :50]
    errs = [np.abs(pc.jpeg_roundtrip(im, q).astype(int) - im).mean() for q in (10, 50, 95)]
    assert errs[0] > errs[1] > errs[2] > 0                                         # lossy, and less so at a higher quality
    # a partial MCU is padded by replication: the result does not depend on what lies beyond the crop
    big = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    big[:50, :50] = im
    pad = np.minimum(np.arange(64), 49)
    assert np.array_equal(pc.jpeg_roundtrip(im, 50), pc.jpeg_roundtrip(big[pad][:, pad], 50)[:50, :50])


def test_jpeg_is_closer_to_pil_than_the_loss_itself():
    """PSNR(restatement, PIL q50 4:2:0) > PSNR(PIL q50, original) on two structured images; the figures, with PIL's neighbouring
    qualities for scale, are the ones recorded in profiles/photometric_parity.json (tools/photometric_parity.py)."""
    pytest.importorskip('PIL')
    from tools import photometric_parity
    fresh = photometric_parity.figures()
    print(json.dumps(fresh))
    for row in fresh['images']:
        assert row['psnr_restatement_vs_pil_q50'] > row['psnr_pil_q50_vs_original'], row
    recorded = json.load(open(os.path.join(ROOT, 'profiles', 'photometric_parity.json')))
    assert len(recorded['images']) == 2 and set(recorded['images'][0]) == set(fresh['images'][0])
    # the record is this run's figures (0.5 dB of slack: another build of PIL's JPEG library may round elsewhere; not a parity bound)
    for rec, row in zip(recorded['images'], fresh['images']):
        assert all(abs(rec[k] - row[k]) <= 0.5 for k in row), (rec, row)


def test_jitter_restatement():
    out = np.zeros((3, 17, 4), np.float32)
    out[..., :2] = 10
    noise = np.full((3, 17, 2), 0.75, np.float32)
    got = pc.jitter_joints(out, 2, noise, 0.5, 0)
    assert (got[:2, :, :2] == 10.25).all() and (got[2] == out[2]).all() and (got[..., 2:] == 0).all()
    assert (pc.jitter_joints(out, 2, noise, 0.5, 1)[:2, :, :2] == 11.25).all()


def test_binding_and_header_carry_the_new_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'og_decoder.h')).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(r'\b' + name + r'\s*\(', text), name
    lib = _lib.load()
    # host-side refusals need no GPU
    assert lib.og_jpeg_roundtrip_batch_u8(None, 1, 16, None, 0, 50, None, None, None, None, None) == _lib.OG_EINVAL
    assert b'null pointer' in lib.og_last_error()


def test_train_dist_has_the_flags():
    from offsetguided_amd import train_dist
    a = train_dist.train_cli([])
    text = open(os.path.join(ROOT, 'offsetguided_amd', 'train_dist.py')).read()
    for flag in ('--color-tint-prob', '--gray-prob', '--jpeg-prob', '--jpeg-quality', '--annotation-jitter-prob'):
        assert flag in text
    assert (a.color_tint_prob, a.gray_prob, a.jpeg_prob, a.jpeg_quality, a.annotation_jitter_prob) == (0, 0, 0, 50, 0)
