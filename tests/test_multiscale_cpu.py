"""CPU-only: the host side of the multi-scale test (--test-scales) -- the affine tables of decoder/multiscale.py, the input chain's
sizes per scale, the command-line validation and the argument checks of og_scale_accumulate_f32."""
import ctypes

import numpy as np
import pytest
import torch

from offsetguided_amd import _lib, evaluate
from offsetguided_amd.decoder import multiscale
from offsetguided_amd.transforms import center_pad_ltrb, initial_meta, multi_scale_sizes, rescale_meta, rescale_size

STRIDE = 4
C0 = STRIDE / 2 - 0.5


def chain_meta(w, h, long_edge, scale):
    """The meta EvalPreprocess.multi_scale writes for one (w, h) image at one scale (rescale + centre pad), host arithmetic only."""
    T, P = multi_scale_sizes(long_edge, scale)
    tw, th = rescale_size(w, h, T)
    meta, _ = rescale_meta(initial_meta(w, h, 7), None, w, h, tw, th)
    ltrb = center_pad_ltrb(tw, th, P, P)
    meta['offset'] = meta['offset'] - np.array(ltrb[:2], np.float64)
    meta['width_height'] = np.array([P, P])
    return meta, (P // STRIDE, P // STRIDE)


@pytest.mark.parametrize('w,h', [(500, 333), (427, 640), (640, 640)])
def test_base_scale_is_the_exact_identity(w, h):
    m, hw = chain_meta(w, h, 640, 1.0)
    aff = multiscale.scale_affines([m, m], [m, m], hw, hw)
    assert aff.dtype == np.float32 and aff.shape == (2, 6)
    assert np.array_equal(aff, np.tile(np.array([1, 0, 1, 0, 1, 1], np.float32), (2, 1)))


@pytest.mark.parametrize('w,h', [(500, 333), (333, 500), (611, 287)])
@pytest.mark.parametrize('scale', [0.5, 1.5, 2.0])
def test_mapped_cell_centres_are_the_same_original_point(w, h, scale):
    mb, hwb = chain_meta(w, h, 640, 1.0)
    ms, hws = chain_meta(w, h, 640, scale)
    Ax, Bx, Ay, By, ix, iy = multiscale.scale_affines([mb], [ms], hwb, hws, dtype=np.float64)[0]
    for ax, (A, B, n) in enumerate(((Ax, Bx, hwb[1]), (Ay, By, hwb[0]))):
        j = np.arange(n, dtype=np.float64)
        x_from_base = (STRIDE * j + C0 + mb['offset'][ax]) / mb['scale'][ax]
        u = A * j + B                                                  # position on the scale-s grid
        x_from_scale = (STRIDE * u + C0 + ms['offset'][ax]) / ms['scale'][ax]
        assert np.abs(x_from_base - x_from_scale).max() <= 1e-9
    # a displacement of d scale-s input pixels is d * sc_b / sc_s base input pixels (offsets are vectors: no translation)
    assert ix == pytest.approx(mb['scale'][0] / ms['scale'][0], abs=0) and iy == pytest.approx(mb['scale'][1] / ms['scale'][1], abs=0)


def test_affines_reject_a_grid_that_does_not_fit_the_meta():
    m, hw = chain_meta(500, 333, 640, 1.0)
    with pytest.raises(ValueError):
        multiscale.scale_affines([m], [m], hw, (hw[0] + 1, hw[1]))


@pytest.mark.parametrize('scale,expected', [(0.5, (320, 384)), (1.0, (640, 640)), (1.5, (960, 1024)), (2.0, (1280, 1280))])
def test_input_sizes_per_scale(scale, expected):
    assert multi_scale_sizes(640, scale) == expected


def test_cli_default_and_parse():
    assert evaluate.evaluate_cli([]).test_scales == [1.0]
    assert evaluate.evaluate_cli(['--test-scales', '0.5', '1', '1.5']).test_scales == [0.5, 1.0, 1.5]
    assert evaluate.evaluate_cli(['--test-scales', '1', '2', '--flip-test']).test_scales == [1.0, 2.0]
    assert evaluate.evaluate_cli(['--test-scales', '1', '--fixed-height']).test_scales == [1.0]   # one scale: today's path


@pytest.mark.parametrize('argv', [
    ['--test-scales', '0', '1'],
    ['--test-scales', '-0.5', '1'],
    ['--test-scales', '1', '1'],
    ['--test-scales', '0.5', '1.5'],
    ['--test-scales', '0.5', '1', '--fixed-height'],
    ['--test-scales', '0.5', '1', '--cat-flip-offset'],
])
def test_cli_rejects(argv):
    with pytest.raises(SystemExit):
        evaluate.evaluate_cli(argv)
    with pytest.raises(ValueError):
        a = [x for x in argv if x.startswith('--') and x != '--test-scales']
        evaluate.validate_test_scales([float(x) for x in argv if not x.startswith('--')], '--fixed-height' in a,
                                      '--cat-flip-offset' in a)


def test_kernel_entry_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    buf = np.zeros(6, np.float32)                # any non-null host address: validation fails before a launch
    p = buf.ctypes.data_as(ctypes.c_void_p)
    rc = lib.og_scale_accumulate_f32(None, p, 1, 0, 17, 19, 8, 8, None, None, None, p, 8, 8, 0, 1.0, p, p, None)
    assert rc == _lib.OG_EINVAL and b'null pointer' in lib.og_last_error()
    rc = lib.og_scale_accumulate_f32(p, p, 1, 1, 17, 19, 8, 8, None, None, None, p, 8, 8, 0, 1.0, p, p, None)
    assert rc == _lib.OG_EINVAL and b'flip tables' in lib.og_last_error()
    rc = lib.og_scale_accumulate_f32(p, p, 1, 0, 17, 19, 8, 8, None, None, None, p, 8, 8, 3, 1.0, p, p, None)
    assert rc == _lib.OG_EINVAL and b'mode 3' in lib.og_last_error()
    rc = lib.og_scale_accumulate_f32(p, p, 1, 0, 17, 19, 0, 8, None, None, None, p, 8, 8, 0, 1.0, p, p, None)
    assert rc == _lib.OG_EINVAL and b'bad shape' in lib.og_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_merge_has_no_cpu_fallback():
    hm, off = torch.zeros(1, 17, 8, 8), torch.zeros(1, 38, 8, 8)
    with pytest.raises(_lib.OgError):
        multiscale.merge_scales([(hm, off)], [np.tile(np.float32([1, 0, 1, 0, 1, 1]), (1, 1))], False, base_hw=(8, 8))
