"""CPU-only: the mask_miss restatement's own properties, the data package on the tiny annotation file, the packed tables, and
og_coco_masks_u8's argument validation (nothing is launched: every refusal comes back without a GPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import coco_mask_common as cm
from offsetguided_amd import _lib, data, train_dist
from offsetguided_amd.config.coco_data import COCO_PERSON_SIGMAS
from offsetguided_amd.data import annotations, masks


def test_rectangle_areas():
    for poly, area in cm.RECT_AREAS:
        assert int(cm.plane_runs(cm.polygon_positions(poly, 29, 37), 29, 37).sum()) == area


def test_xor_form_equals_run_form_on_the_random_set():
    records = cm.random_polygon_records()
    assert len(records) == 300
    for r in records:
        h, w = r['height'], r['width']
        pos = cm.polygon_positions(r['segmentation'][0][0], h, w)
        assert np.array_equal(cm.plane_runs(pos, h, w), cm.plane_xor(pos, h, w))
    for _, h, w, polys in cm.POLYGON_CASES:
        for poly in polys:
            pos = cm.polygon_positions(poly, h, w)
            assert np.array_equal(cm.plane_runs(pos, h, w), cm.plane_xor(pos, h, w))


def test_directed_polygons_behave_as_named():
    got = {name: cm.annotation_mask(polys, h, w) for name, h, w, polys in cm.POLYGON_CASES}
    assert np.array_equal(got['triangle steep + shallow'], got['triangle, other winding'])
    assert not got['wholly outside'].any() and not got['one vertex'].any() and not got['two vertices'].any()
    clamped = got['clamped to y = h: a toggle on the next column']
    assert clamped[20:, 4:15].all() and int(clamped.sum()) == 9 * 11          # an in-column-only fill would spill into column 15
    assert got['clamped in the last column: a toggle at h w'][10:, 30:].all()
    union = got['two overlapping polygons: a union']
    assert union[20, 20] and int(union.sum()) == 20 * 20 + 25 * 22 - 10 * 10
    assert got['1 x 1 covered'].all() and not got['1 x 1 missed'].any()


def test_string_decode_equals_the_list():
    runs = [500, 300, 20, 400, 1, 1851]
    tiny = cm.tiny_json()
    s = [a for a in tiny['annotations'] if isinstance(a['segmentation'], dict) and isinstance(a['segmentation']['counts'], str)][0]
    s = s['segmentation']['counts']
    assert cm.string_to_runs(s) == runs and data.rle_counts(s) == runs and cm.runs_to_string(runs) == s
    for seq in ([0, 5, 3, 900, 2, 0, 7], [3072], [1, 2, 3, 100000, 2, 50000, 1]):
        assert data.rle_counts(cm.runs_to_string(seq)) == seq == cm.string_to_runs(cm.runs_to_string(seq))
    assert data.rle_counts([4, 5]) == [4, 5]
    with pytest.raises(ValueError):
        data.rle_counts('d')                  # the continue bit set on the last character


def test_load_annotations_on_the_tiny_file():
    from offsetguided_amd import cocoeval
    recs = data.load_annotations(cm.GOLDEN)
    gt = cocoeval.load_ground_truth(cm.GOLDEN)
    assert list(recs) == [101, 102, 103, 104, 105, 106] == list(gt)
    for image_id, rec in recs.items():
        assert set(gt[image_id]) == {'keypoints', 'area', 'bbox', 'iscrowd', 'num_keypoints'}          # the scorer's entry is unchanged
        for key, value in gt[image_id].items():
            assert np.array_equal(rec[key], value) and rec[key].dtype == value.dtype
        assert len(rec['segmentation']) == len(rec['area'])
    assert [len(r['area']) for r in recs.values()] == [3, 5, 2, 1, 0, 1]           # the category-2 annotation of image 105 is not a person
    assert (recs[101]['height'], recs[101]['width'], recs[101]['file_name']) == (29, 37, 'img_101.png')
    assert list(recs[102]['iscrowd']) == [0, 0, 0, 1, 1] and isinstance(recs[102]['segmentation'][3]['counts'], str)


def test_normalize_annotations():
    recs = data.load_annotations(cm.GOLDEN)
    kp = data.normalize_annotations(recs[102])
    assert kp.shape == (2, 17, 4) and kp.dtype == np.float32      # the person without keypoints and the two crowds are gone
    anns = [a for a in cm.tiny_json()['annotations'] if a['image_id'] == 102]
    small, normal = anns[1], anns[2]
    assert small['area'] == 1024 and (kp[0, :, 2] == 0).all()     # area <= 32 * 32: no keypoint counts
    assert np.array_equal(kp[0, :, :2], np.asarray(small['keypoints'], np.float32).reshape(17, 3)[:, :2])
    assert np.array_equal(kp[1, :, :3], np.asarray(normal['keypoints'], np.float32).reshape(17, 3))
    want = (np.sqrt(normal['bbox'][3] * normal['bbox'][2]) * np.array(COCO_PERSON_SIGMAS)).astype(np.float32)
    assert np.array_equal(kp[1, :, 3], want)
    assert data.normalize_annotations(recs[105]).shape == (0, 17, 4)


def _write_images(tmp_path, recs):
    from PIL import Image
    for rec in recs.values():
        rs = np.random.RandomState(rec['image_id'])
        Image.fromarray(rs.randint(0, 256, (rec['height'], rec['width'], 3)).astype(np.uint8)).save(tmp_path / rec['file_name'])


def test_coco_keypoints_id_filtering_and_items(tmp_path):
    recs = data.load_annotations(cm.GOLDEN)
    _write_images(tmp_path, recs)
    ds = data.CocoKeypoints(str(tmp_path), cm.GOLDEN)
    assert ds.ids == [101, 102, 103, 104]                         # 105 has no person, 106 a person without a labelled keypoint
    assert data.CocoKeypoints(str(tmp_path), cm.GOLDEN, all_persons=True).ids == [101, 102, 103, 104, 106]
    assert data.CocoKeypoints(str(tmp_path), cm.GOLDEN, all_images=True).ids == [101, 102, 103, 104, 105, 106]
    assert data.CocoKeypoints(str(tmp_path), cm.GOLDEN, n_images=2).ids == [101, 102]
    image, rec, meta = ds[0]
    assert image.shape == (29, 37, 3) and image.dtype == np.uint8 and rec is ds.annotations[101]
    assert np.array_equal(image, np.random.RandomState(101).randint(0, 256, (29, 37, 3)).astype(np.uint8))
    assert meta == {'dataset_index': 0, 'image_id': 101, 'file_name': 'img_101.png', 'image_path': os.path.join(str(tmp_path), 'img_101.png'),
                    'flickr_full_page': 'http://flickr.com/photo.gne?id=1234567'}
    assert set(ds[1][2]) == {'dataset_index', 'image_id', 'file_name', 'image_path'}
    strict = data.CocoKeypoints(str(tmp_path), cm.GOLDEN, strict_crowd=True)
    strict[0]                                                     # one crowd: served
    with pytest.raises(Exception, match='crowd segments > 1'):
        strict[1]
    with pytest.raises(IOError):
        data.CocoKeypoints(str(tmp_path / 'nowhere'), cm.GOLDEN)[0]
    listed = data.ImageList([str(tmp_path / 'img_104.png')])
    image, anns, meta = listed[0]
    assert image.shape == (1, 1, 3) and anns == [] and meta['dataset_index'] == 0 and len(listed) == 1
    batches = list(data.raw_batches(ds, 3))
    assert [len(b[0]) for b in batches] == [3, 1] and [m['image_id'] for m in batches[0][2]] == [101, 102, 103]


def test_collate_raw_tables(tmp_path):
    recs = data.load_annotations(cm.GOLDEN)
    _write_images(tmp_path, recs)
    ds = data.CocoKeypoints(str(tmp_path), cm.GOLDEN, all_images=True)
    images, joints, n_persons, tables, metas = data.collate_raw([ds[i] for i in range(len(ds))])
    assert len(images) == 6 and joints.shape == (6, 2, 17, 4) and list(n_persons) == [2, 2, 2, 1, 0, 0]
    assert [m['image_id'] for m in metas] == [101, 102, 103, 104, 105, 106]
    assert tables.sizes == [(29, 37), (48, 64), (33, 31), (1, 1), (29, 37), (33, 31)]
    assert tables.offsets == list(np.cumsum([0] + [h * w for h, w in tables.sizes[:-1]])) and tables.out_bytes == sum(h * w for h, w in tables.sizes)
    assert tables.counts == (6, 12, 15, 41, 19)          # 41 vertices, 10 + 6 + 3 runs
    at = tables.at
    assert all(a % 16 == 0 for a in at)
    im = tables.buffer[at[0]:at[0] + 6 * annotations.IMAGE_DT.itemsize].view(annotations.IMAGE_DT)
    assert list(im['n_anns']) == [3, 5, 2, 1, 0, 1] and list(im['ann_first']) == [0, 3, 8, 10, 11, 11] and list(im['out_off']) == tables.offsets
    an = tables.buffer[at[1]:at[1] + 12 * annotations.ANN_DT.itemsize].view(annotations.ANN_DT)
    assert list(an['flags']) == [0, 1, 0, 2, 2, 0, 1, 1, 0, 0, 2, 2] and list(an['n_pieces']) == [1, 1, 1, 1, 1, 2, 1, 1, 2, 2, 1, 1]
    pc = tables.buffer[at[2]:at[2] + 15 * annotations.PIECE_DT.itemsize].view(annotations.PIECE_DT)
    words = [(h * w + 31) // 32 for h, w in tables.sizes]
    assert list(pc['word_off']) == list(np.cumsum([0] + [words[i] for i in pc['image'][:-1]]))
    assert list(pc['kind'][[1, 7, 8]]) == [1, 1, 1] and int(pc['kind'].sum()) == 3
    cums = tables.buffer[at[4]:at[4] + 19 * 4].view(np.uint32)
    assert list(cums[:10]) == list(np.cumsum([0, 40, 0, 0, 30, 200, 0, 5, 100, 698])) and cums[9] == 29 * 37
    with pytest.raises(ValueError, match='odd number'):
        data.mask_tables([cm.record(8, 8, [([[1, 2, 3]], 0, 1, 2000.0)])])
    with pytest.raises(ValueError, match='RLE of size'):
        data.mask_tables([cm.record(8, 8, [({'size': [8, 9], 'counts': [72]}, 1, 0, 10.0)])])


def _desc(tables, dev=16, miss=16, every=16):
    """A descriptor over the tables' own buffer; the device pointers are never dereferenced: every call below is refused first."""
    return masks.descriptor(tables, tables.buffer.ctypes.data, dev, miss, every)


def test_argument_validation_without_gpu():
    lib = _lib.load()
    good = lambda: data.mask_tables(cm.tiny_records())                                                  # noqa: E731

    def refused(tables, text, **kw):
        desc = _desc(tables, **kw)
        rc = lib.og_coco_masks_u8(C.byref(desc), C.c_void_p(16), 1 << 30, None)
        assert rc == _lib.OG_EINVAL and text in lib.og_last_error(), lib.og_last_error()

    t = good()
    assert lib.og_coco_mask_workspace_bytes(C.byref(_desc(t))) >= 4 * sum((h * w + 31) // 32 for h, w in
                                                                          [t.sizes[i] for i in (0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 5)])
    assert lib.og_coco_masks_u8(None, C.c_void_p(16), 1 << 30, None) == _lib.OG_EINVAL and b'null pointer' in lib.og_last_error()
    refused(t, b'null pointer', dev=None)
    refused(t, b'null pointer', miss=None)
    desc = _desc(t)
    assert lib.og_coco_masks_u8(C.byref(desc), None, 1 << 30, None) == _lib.OG_EINVAL and b'null pointer' in lib.og_last_error()
    assert lib.og_coco_masks_u8(C.byref(desc), C.c_void_p(16), 64, None) == _lib.OG_ENOSPC
    desc.size -= 8
    assert lib.og_coco_masks_u8(C.byref(desc), C.c_void_p(16), 1 << 30, None) == _lib.OG_EINVAL and b'descriptor size' in lib.og_last_error()
    assert lib.og_coco_mask_workspace_bytes(C.byref(desc)) == 0
    t = good()
    t.counts = (0,) + t.counts[1:]
    refused(t, b'n_images')
    t = good()
    t.counts = t.counts[:2] + (-1,) + t.counts[3:]
    refused(t, b'negative count')
    for h, w, text in ((0, 5, b'has size'), (5, -1, b'has size'), (1 << 14, (1 << 14) + 1, b'beyond 2^28')):
        t = data.mask_tables([cm.record(h, w, [])])
        refused(t, text)
    refused(data.mask_tables([cm.record(8, 8, [([[]], 0, 1, 2000.0)])]), b'fewer than 1 vertex')
    for bad in (float('nan'), float('inf'), -float('inf')):
        refused(data.mask_tables([cm.record(8, 8, [([[1.0, 2.0, bad, 3.0, 4.0, 5.0]], 0, 1, 2000.0)])]), b'non-finite vertex')
    refused(data.mask_tables([cm.record(8, 8, [([[1.0, 2.0, 3e7, 3.0, 4.0, 5.0]], 0, 1, 2000.0)])]), b'beyond 2^20')
    refused(data.mask_tables([cm.record(8, 8, [({'size': [8, 8], 'counts': [10, 20, 33]}, 1, 0, 10.0)])]), b'sum to 63')
    refused(data.mask_tables([cm.record(8, 8, [({'size': [8, 8], 'counts': [10, 20, 35]}, 1, 0, 10.0)])]), b'sum to 65')
    t = good()
    t.out_bytes -= 1
    refused(t, b'output bytes')


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check")
def test_device_masks_needs_a_gpu():
    tables = data.mask_tables(cm.tiny_records())
    with pytest.raises(_lib.OgError):
        data.device_masks(tables, 'cpu')
    with pytest.raises(_lib.OgError):
        data.device_masks(tables, 'cuda:0')


def test_train_parser_takes_the_new_flags_and_defaults_to_today(tmp_path):
    args = train_dist.train_cli(['--no-pretrain'])
    assert args.train_annotations is None and args.train_image_dir is None and args.augment is False
    args = train_dist.train_cli(['--no-pretrain', '--train-annotations', cm.GOLDEN, '--train-image-dir', str(tmp_path)])
    assert args.train_annotations == cm.GOLDEN and args.train_image_dir == str(tmp_path) and args.augment is True
    with pytest.raises(SystemExit):
        train_dist.train_cli(['--no-pretrain', '--train-annotations', cm.GOLDEN])
    # without a mask the encoders are called exactly as before: (joints, n_persons), no third argument
    calls = []

    class Enc:
        def encode_batch(self, *a):
            calls.append(a)
            e = torch.zeros(0)
            return e, e, e, 'mask%d' % len(a)
    out = train_dist.encode_targets([Enc(), Enc()], 'j', 'n')
    assert calls == [('j', 'n'), ('j', 'n')] and out[0][3] == out[1][3] == 'mask2'
    del calls[:]
    out = train_dist.encode_targets([Enc(), Enc()], 'j', 'n', mask_miss='m')
    assert calls == [('j', 'n', 'm'), ('j', 'n', 'm')] and out[0][3] == 'mask3'
