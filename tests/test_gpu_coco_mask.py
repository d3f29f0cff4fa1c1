"""GPU: og_coco_masks_u8 (csrc/coco_mask.hip) bit for bit against the numpy restatement (tests/coco_mask_common.py, the
sort-and-merge run-length form) on the directed cases, the tiny annotation file and 300 random polygons; and the mask's way through
DeviceAugment, the encoders and one training step."""
import copy
import ctypes as C
import random

import numpy as np
import pytest
import torch

import coco_mask_common as cm
from offsetguided_amd import _lib, data, encoder, train_dist, transforms
from offsetguided_amd.data import masks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def _check(records, key, dev, mask_all=True):
    want = cm.reference_masks(key, records)
    got = data.device_masks(data.mask_tables(records), dev, mask_all=mask_all)
    assert len(got) == len(records) and (got.mask_all is None) == (not mask_all)
    for i, (miss, every) in enumerate(want):
        assert torch.equal(got.plane(i).cpu(), torch.from_numpy(np.array(miss))), (key, i, 'mask_miss')
        if mask_all:
            assert torch.equal(got.plane(i, 'mask_all').cpu(), torch.from_numpy(np.array(every))), (key, i, 'mask_all')
    return got


def test_directed_polygons(dev):
    _check(cm.polygon_case_records(), 'polygons', dev)


def test_tiny_file_in_one_batch_of_mixed_sizes(dev):
    records = cm.tiny_records()
    got = _check(records, 'tiny', dev)
    _check(records, 'tiny', dev, mask_all=False)
    # the crowd of image 101 sits between two persons it overlaps: where it covers the first it is taken back, where the second it stays
    miss, every = got.plane(0).cpu().numpy(), got.plane(0, 'mask_all').cpu().numpy()
    first, crowd = cm.annotation_mask(records[0]['segmentation'][0], 29, 37), cm.annotation_mask(records[0]['segmentation'][1], 29, 37)
    second = cm.annotation_mask(records[0]['segmentation'][2], 29, 37)
    assert (first & crowd).any() and (miss[first & crowd] == 255).all()
    assert (second & crowd & ~first).any() and (miss[second & crowd & ~first] == 0).all() and (every[crowd] == 255).all()
    # no annotations: everything labelled, nobody there
    assert (got.plane(4).cpu().numpy() == 255).all() and (got.plane(4, 'mask_all').cpu().numpy() == 0).all()


def test_directed_and_tiny_together(dev):
    _check(cm.polygon_case_records() + cm.tiny_records(), 'polygons+tiny', dev)


def test_random_polygons_fifty_to_a_call(dev):
    records = cm.random_polygon_records()
    assert len(records) == 300
    for first in range(0, 300, 50):
        _check(records[first:first + 50], ('random', first), dev, mask_all=first % 100 == 0)


def test_dirty_workspace_gives_the_same_bits(dev):
    """The raw entry point twice on one workspace, filled with ones before the first call and left as it is before the second."""
    lib = _lib.load()
    records = cm.tiny_records() + cm.polygon_case_records()
    tables = data.mask_tables(records)
    dev_tables = torch.from_numpy(tables.buffer).to(dev)
    outs = []
    ws = None
    for _ in range(2):
        miss = torch.zeros(tables.out_bytes, dtype=torch.uint8, device=dev)
        every = torch.zeros(tables.out_bytes, dtype=torch.uint8, device=dev)
        desc = masks.descriptor(tables, tables.buffer.ctypes.data, dev_tables, miss, every)
        if ws is None:
            ws = torch.full((lib.og_coco_mask_workspace_bytes(C.byref(desc)),), 0xff, dtype=torch.uint8, device=dev)
        _lib.check(lib.og_coco_masks_u8(C.byref(desc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
        outs.append((miss.cpu(), every.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want = cm.reference_masks('tiny+polygons', records)
    assert torch.equal(outs[1][0], torch.from_numpy(np.concatenate([m.reshape(-1) for m, _ in want])))
    assert torch.equal(outs[1][1], torch.from_numpy(np.concatenate([a.reshape(-1) for _, a in want])))


def _tiny_batch(n=2):
    records = cm.tiny_records()[:n]
    images = [np.random.RandomState(r['image_id']).randint(0, 256, (r['height'], r['width'], 3)).astype(np.uint8) for r in records]
    batch = [(im, r, {'image_id': r['image_id']}) for im, r in zip(images, records)]
    return data.collate_raw(batch), records


def test_device_masks_and_augment_never_wait(dev):
    (images, joints, n_persons, tables, _), records = _tiny_batch(4)
    S = 64
    aug = transforms.DeviceAugment(S, transforms.AugParams(max_translate=8), device=dev)
    for _ in range(3):                                    # allocator, pinned staging buffers, the workspace, library warm-up
        aug(images, joints, n_persons, data.device_masks(tables, dev), rng=random.Random(1))
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        dm = data.device_masks(tables, dev)
        out, jout, mout, mats = aug(images, joints, n_persons, dm, rng=random.Random(11))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    # the same planes as host arrays give the same warped mask, bit for bit
    host = [dm.plane(i).cpu().numpy() for i in range(len(dm))]
    for plane, (miss, _) in zip(host, cm.reference_masks('tiny4', records)):
        assert np.array_equal(plane, miss)
    out2, jout2, mout2, mats2 = aug(images, joints, n_persons, host, rng=random.Random(11))
    assert np.array_equal(mats, mats2) and torch.equal(out, out2) and torch.equal(jout, jout2)
    assert mout.shape == (4, S, S) and mout.dtype == torch.uint8 and torch.equal(mout, mout2)
    assert bool((mout == 0).any()) and bool((mout == 255).any())


class TinyNet(torch.nn.Module):
    """Stand-in with the NetworkWrapper output nesting (tests/test_train_step.py): the step's subject here is the mask, not the backbone."""

    def __init__(self):
        super().__init__()
        self.body = torch.nn.Conv2d(3, 8, 3, stride=4, padding=1)
        self.hm = torch.nn.ModuleList([torch.nn.Conv2d(8, 17, 1) for _ in range(2)])
        self.off = torch.nn.ModuleList([torch.nn.Conv2d(8, 38, 1) for _ in range(2)])

    def forward(self, x):
        f = torch.relu(self.body(x))
        return [([h(f) for h in self.hm], [[], []], [[], []]), ([o(f) for o in self.off], [[], []], [[], []])]


def test_mask_reaches_the_encoders_and_the_losses(dev, monkeypatch):
    from offsetguided_amd.models import losses
    (images, joints, n_persons, tables, _), _ = _tiny_batch(2)
    S = train_dist.train_cli(['--no-pretrain', '--square-length', '128']).square_length
    monkeypatch.setattr(encoder.HeatMaps, 'include_jitter_offset', False)
    monkeypatch.setattr(encoder.HeatMaps, 'include_background', False)
    monkeypatch.setattr(encoder.OffsetMaps, 'include_scale', False)
    encs = encoder.factory_heads(['hmp', 'omp'], S, [4, 4], dev)
    aug = transforms.DeviceAugment(S, transforms.FixedAugParams(), device=dev)
    entry = (images, joints, n_persons, torch.from_numpy(n_persons).to(dev), tables)
    crops, annos = train_dist.augmented_batch(aug, entry, random.Random(5))
    assert len(annos) == 3 and annos[2].shape == (2, S, S) and annos[2].dtype == torch.uint8
    crops_plain, annos_plain = train_dist.augmented_batch(aug, entry[:4], random.Random(5))
    assert len(annos_plain) == 2 and torch.equal(crops, crops_plain) and torch.equal(annos[0], annos_plain[0])
    masked = train_dist.encode_targets(encs, *annos)
    plain = train_dist.encode_targets(encs, *annos_plain)
    lib = _lib.load()
    shrunk = torch.empty((2, 1, S // 4, S // 4), dtype=torch.uint8, device=dev)
    _lib.check(lib.og_shrink_mask_miss_u8(_lib.ptr(annos[2]), 2, S, S, 4, _lib.ptr(shrunk), _lib.stream_ptr(dev)), lib)
    assert torch.equal(masked[0][3], shrunk.bool()) and torch.equal(masked[1][3], shrunk.bool())
    assert bool(plain[0][3].all()) and not bool(masked[0][3].all()) and bool(masked[0][3].any())
    assert torch.equal(masked[0][0], plain[0][0]) and torch.equal(masked[1][0], plain[1][0])          # the targets themselves do not move
    crit = losses.lossfuncs_factory(['hmp', 'omp'], 2, [1, 1], 'focal_l2_loss', 'offset_l1_loss', 'offset_instance_l1_loss',
                                    'scale_l1_loss', True)
    torch.manual_seed(0)
    net = TinyNet().to(dev)
    twin = copy.deepcopy(net)
    step = lambda model, targets: train_dist.train_step(model, crit, torch.optim.Adam(model.parameters(), lr=1e-3), crops, targets,  # noqa: E731
                                                        [1, 0, 0, 100, 0.01], autocast_dtype=None)
    loss_masked, _ = step(net, masked)
    loss_plain, _ = step(twin, plain)
    assert np.isfinite(float(loss_masked)) and np.isfinite(float(loss_plain))
    assert float(loss_masked) != float(loss_plain)
