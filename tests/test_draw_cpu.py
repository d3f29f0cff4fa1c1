"""CPU: the pose painter's numpy restatement (tests/draw_common.py) checked against itself and against hand-computed pictures, the PPM
writer, and the command line.  The HIP kernel is held to the fp32 restatement bit for bit in tests/test_gpu_draw.py."""
import numpy as np
import pytest

from draw_common import CASES, TOY, draw_reference, reference
from offsetguided_amd import evaluate, visualization


@pytest.mark.parametrize('name', sorted(CASES))
def test_fp32_restatement_within_one_level_of_fp64(name):
    """Positions carry at most ~1e-4 px of fp32 error (coordinates < 128 px: ulp 8e-6, a dozen operations), the blend a few 1e-5 of a
    level per primitive: < 0.03 level before the final rounding, which can then land on either side of a .5 -- at most one level."""
    a, b = reference(name, np.float32), reference(name, np.float64)
    diff = np.abs(a.astype(np.int16) - b.astype(np.int16))
    assert diff.max() <= 1, (name, int(diff.max()))
    assert (a != CASES[name]['images']).any(), 'the case paints nothing'


def test_horizontal_one_pixel_segment_paints_exactly_its_row():
    img = np.full((1, 9, 20, 3), 7, np.uint8)
    poses = np.array([[[(3.0, 4.0, 1.0), (15.0, 4.0, 1.0), (0.0, 0.0, 0.0)]]], np.float32)        # one limb, no visible third keypoint
    colour = np.array([[200, 100, 50]], np.uint8)
    out = draw_reference(img, poses, [1], [(0, 1)], colour, 1.0, 0.0, 1.0, np.float32)           # r = 0.5: cov = 1 - d; marker radius 0
    assert (out[0, 4, 3:16] == colour[0]).all()                   # d = 0 on the row between the end points: full colour
    assert (out[0, 2] == 7).all() and (out[0, 6] == 7).all()      # two rows away: d = 2, untouched
    assert (out[0, 3] == 7).all() and (out[0, 5] == 7).all()      # one row away: d = 1, cov = 0
    assert (out[0, 4, :3] == 7).all() and (out[0, 4, 16:] == 7).all()    # beyond the caps: d >= 1


def test_order_of_persons_matters_with_alpha():
    img = np.zeros((1, 12, 24, 3), np.uint8)
    a = np.array([(12.0, 6.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)], np.float32)     # one visible keypoint each: a single disc
    b = np.array([(13.0, 6.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)], np.float32)
    pal = np.array([[255, 0, 0], [0, 0, 255]], np.uint8)
    ab = draw_reference(img, np.stack([a, b])[None], [2], TOY, pal, 2.0, 3.0, 0.5, np.float32)
    ba = draw_reference(img, np.stack([b, a])[None], [2], TOY, pal[::-1], 2.0, 3.0, 0.5, np.float32)    # same colours per pose, other order
    assert (ab != ba).any()
    assert (ab[0, 6, 12] == [64, 0, 128]).all() and (ba[0, 6, 12] == [128, 0, 64]).all()    # 0 -> 127.5 -> 63.75 / 127.5: the later one wins


def test_save_ppm_round_trip(tmp_path):
    img = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    path = visualization.save_ppm(str(tmp_path / 'x.ppm'), img)
    raw = open(path, 'rb').read()
    fields, pos = [], 0
    while len(fields) < 4:                                   # magic, width, height, maxval: whitespace-separated, one byte after the last
        while raw[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while not raw[end:end + 1].isspace():
            end += 1
        fields.append(raw[pos:end])
        pos = end
    assert fields[0] == b'P6' and [int(f) for f in fields[1:]] == [7, 5, 255]
    body = raw[pos + 1:]
    assert len(body) == 5 * 7 * 3 and (np.frombuffer(body, np.uint8).reshape(5, 7, 3) == img).all()
    with pytest.raises(ValueError):
        visualization.save_ppm(str(tmp_path / 'y.ppm'), img.astype(np.float32))


def test_tab20_table():
    assert visualization.TAB20.shape == (20, 3) and visualization.TAB20.dtype == np.uint8
    assert len({tuple(c) for c in visualization.TAB20.tolist()}) == 20


def test_cli_accepts_show_dir():
    a = evaluate.evaluate_cli(['--no-pretrain', '--show-detected-poses', '--show-dir', 'somewhere'])
    assert a.show_detected_poses and a.show_dir == 'somewhere'
    a = evaluate.evaluate_cli(['--no-pretrain'])
    assert not a.show_detected_poses and a.show_dir == '.'
