"""GPU: og_coco_masks_u8 (csrc/coco_mask.hip) bit for bit against the numpy restatement (tests/coco_mask_common.py) on planes of
more than one 256-word chunk (tests/coco_mask_large_cases.py): the fill's carry from chunk to chunk, the lanes' further passes over
long RLEs and long edges, COCO-size images, and a batch of unequal images through the compose grid."""
import ctypes as C

import numpy as np
import pytest
import torch

import coco_mask_common as cm
import coco_mask_large_cases as lc
from offsetguided_amd import _lib, data
from offsetguided_amd.data import masks

pytestmark = pytest.mark.gpu

GUARD = 64          # bytes of 0x77 on either side; a multiple of 16 keeps the workspace aligned


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def _check(records, want, dev, mask_all=True):
    got = data.device_masks(data.mask_tables(records), dev, mask_all=mask_all)
    assert len(got) == len(records) == len(want) and (got.mask_all is None) == (not mask_all)
    for i, (r, (miss, every)) in enumerate(zip(records, want)):
        assert torch.equal(got.plane(i).cpu(), torch.from_numpy(np.array(miss))), (i, r['name'], 'mask_miss')
        if mask_all:
            assert torch.equal(got.plane(i, 'mask_all').cpu(), torch.from_numpy(np.array(every))), (i, r['name'], 'mask_all')


def _check_group(group, dev, **kw):
    _check(lc.GROUPS[group](), lc.reference(group), dev, **kw)


def test_chunk_boundaries_in_one_call(dev):
    _check_group('chunk boundaries', dev)


def test_chunk_boundaries_each_alone(dev):
    for r, want in zip(lc.chunk_boundary_records(), lc.reference('chunk boundaries')):
        _check([r], [want], dev)


def test_directed_toggles(dev):
    _check_group('directed toggles', dev)


def test_whole_image_covered(dev):
    _check_group('whole image', dev)


def test_long_rles(dev):
    _check_group('long RLEs', dev)


def test_long_edges(dev):
    _check_group('long edges', dev)


def test_coco_sizes_in_one_batch_of_unequal_images(dev):
    _check_group('COCO sizes', dev)
    _check_group('COCO sizes', dev, mask_all=False)
    # the largest image last, and alone behind the smallest: the compose grid is sized by the largest, wherever it stands
    records, want = lc.coco_size_records(), lc.reference('COCO sizes')
    _check(records[::-1], want[::-1], dev)
    _check([records[3], records[2]], [want[3], want[2]], dev)


def test_random_polygons_at_size(dev):
    _check_group('random at size', dev)


def _flat(want, which):
    return torch.from_numpy(np.concatenate([pair[which].reshape(-1) for pair in want]))


def _raw(tables, dev):
    """(device tables, guarded mask_miss, guarded mask_all, a descriptor over them): every buffer exactly the size the tables name."""
    dev_tables = torch.from_numpy(tables.buffer).to(dev)
    outs = [torch.full((tables.out_bytes + 2 * GUARD,), 0x77, dtype=torch.uint8, device=dev) for _ in range(2)]
    desc = masks.descriptor(tables, tables.buffer.ctypes.data, dev_tables, outs[0][GUARD:], outs[1][GUARD:])
    return dev_tables, outs[0], outs[1], desc


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0x77).all()) and bool((buf[-GUARD:] == 0x77).all())


def test_dirty_workspace_gives_the_same_bits_at_coco_size(dev):
    """The raw entry point twice on one workspace, filled with ones before the first call and left as it is before the second."""
    lib = _lib.load()
    tables = data.mask_tables(lc.coco_size_records())
    want = lc.reference('COCO sizes')
    ws = None
    for _ in range(2):
        dev_tables, miss, every, desc = _raw(tables, dev)
        if ws is None:
            ws = torch.full((lib.og_coco_mask_workspace_bytes(C.byref(desc)),), 0xff, dtype=torch.uint8, device=dev)
        _lib.check(lib.og_coco_masks_u8(C.byref(desc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
        assert torch.equal(miss[GUARD:-GUARD].cpu(), _flat(want, 0)) and torch.equal(every[GUARD:-GUARD].cpu(), _flat(want, 1))


def test_guard_bytes_round_outputs_and_workspace(dev):
    lib = _lib.load()
    tables = data.mask_tables(lc.coco_size_records())
    want = lc.reference('COCO sizes')
    dev_tables, miss, every, desc = _raw(tables, dev)
    ws_bytes = lib.og_coco_mask_workspace_bytes(C.byref(desc))
    words = sum((r['height'] * r['width'] + 31) // 32 * len(lc.pieces(r)) for r in lc.coco_size_records())
    assert ws_bytes == (4 * words + 15) // 16 * 16 + 16 and tables.out_bytes == 2 * 480 * 640 + 427 * 640 + 1
    ws = torch.full((ws_bytes + 2 * GUARD,), 0x77, dtype=torch.uint8, device=dev)
    assert ws[GUARD:].data_ptr() % 16 == 0
    _lib.check(lib.og_coco_masks_u8(C.byref(desc), _lib.ptr(ws[GUARD:]), ws_bytes, _lib.stream_ptr(dev)), lib)
    assert torch.equal(miss[GUARD:-GUARD].cpu(), _flat(want, 0)) and torch.equal(every[GUARD:-GUARD].cpu(), _flat(want, 1))
    assert _guards_intact(miss) and _guards_intact(every) and _guards_intact(ws)
    assert lib.og_coco_masks_u8(C.byref(desc), _lib.ptr(ws[GUARD:]), ws_bytes - 1, _lib.stream_ptr(dev)) == _lib.OG_ENOSPC


def test_stages_one_by_one_give_the_bits_of_one_call(dev):
    lib = _lib.load()
    records = lc.coco_size_records()[2:] + lc.directed_toggle_records()[-5:] + lc.long_edge_records()[-3:]
    want = lc.reference('COCO sizes')[2:] + lc.reference('directed toggles')[-5:] + lc.reference('long edges')[-3:]
    tables = data.mask_tables(records)
    dev_tables, miss, every, desc = _raw(tables, dev)
    ws = torch.full((lib.og_coco_mask_workspace_bytes(C.byref(desc)),), 0xff, dtype=torch.uint8, device=dev)
    for stage in (1, 2, 4, 8):          # zero, toggle, fill, compose
        desc.stages = stage
        _lib.check(lib.og_coco_masks_u8(C.byref(desc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
        if stage < 8:                   # nothing but compose writes an output
            assert bool((miss == 0x77).all()) and bool((every == 0x77).all())
    staged = miss[GUARD:-GUARD].cpu(), every[GUARD:-GUARD].cpu()
    assert torch.equal(staged[0], _flat(want, 0)) and torch.equal(staged[1], _flat(want, 1))
    dev_tables, miss, every, desc = _raw(tables, dev)
    _lib.check(lib.og_coco_masks_u8(C.byref(desc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
    assert torch.equal(miss[GUARD:-GUARD].cpu(), staged[0]) and torch.equal(every[GUARD:-GUARD].cpu(), staged[1])
    assert _guards_intact(miss) and _guards_intact(every)
