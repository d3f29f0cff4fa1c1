"""mask_miss / mask_all of a batch on the device (csrc/coco_mask.hip): one pinned copy of the tables, og_coco_masks_u8's launches on
the current stream, no wait.  There is no CPU path."""
import ctypes as C

import torch

from .. import _lib


class DeviceMasks:
    """Packed row-major (h, w) uint8 planes (0 / 255) on the device: `buffer` holds mask_miss, image i at byte offsets[i] with
    sizes[i] = (h, w) -- the masks / offsets form og_warp_affine_mask_u8 takes --, `mask_all` the same layout or None.  Everything
    was queued on the stream that was current in device_masks(): use it on that stream, or order the streams."""

    def __init__(self, buffer, offsets, sizes, mask_all=None, keep=None):
        self.buffer, self.offsets, self.sizes, self.mask_all = buffer, list(offsets), list(sizes), mask_all
        self._keep = keep      # the pinned tables: the copy that reads them is queued, not done

    def __len__(self):
        return len(self.sizes)

    def plane(self, i, which='mask_miss'):
        """(h, w) view of image i's plane; which: 'mask_miss' or 'mask_all'."""
        src = self.buffer if which == 'mask_miss' else self.mask_all
        h, w = self.sizes[i]
        return src[self.offsets[i]:self.offsets[i] + h * w].view(h, w)


def descriptor(tables, host_ptr, dev_ptr, mask_miss, mask_all):
    n_images, n_anns, n_pieces, n_vertices, n_cums = tables.counts
    return _lib.CocoMaskDesc(n_images=n_images, n_anns=n_anns, n_pieces=n_pieces, n_vertices=n_vertices, n_cums=n_cums,
                             tables_host=host_ptr, tables_dev=dev_ptr, table_bytes=tables.buffer.nbytes, images_at=tables.at[0],
                             anns_at=tables.at[1], pieces_at=tables.at[2], vertices_at=tables.at[3], cums_at=tables.at[4],
                             mask_miss=mask_miss, mask_all=mask_all, out_bytes=tables.out_bytes)


def device_masks(tables, device, mask_all=True):
    """annotations.MaskTables (collate_raw's) -> DeviceMasks.  Raises OgError without a GPU, like every other product path."""
    device = torch.device(device)
    if device.type != 'cuda' or not torch.cuda.is_available():
        raise _lib.OgError(f'device_masks: device is {device}; the HIP kernels need a GPU (offsetguided_amd has no CPU path)')
    lib = _lib.load()
    pinned = torch.empty(tables.buffer.nbytes, dtype=torch.uint8).pin_memory()
    pinned.numpy()[:] = tables.buffer
    dev_tables = pinned.to(device, non_blocking=True)
    miss = torch.empty(max(tables.out_bytes, 16), dtype=torch.uint8, device=device)
    every = torch.empty(max(tables.out_bytes, 16), dtype=torch.uint8, device=device) if mask_all else None
    desc = descriptor(tables, pinned.data_ptr(), dev_tables, miss, every)
    ws_bytes = lib.og_coco_mask_workspace_bytes(C.byref(desc))
    if ws_bytes == 0:
        _lib.check(_lib.OG_EINVAL, lib)
    ws = _lib.workspace(device, ws_bytes, tag='coco_mask')
    _lib.check(lib.og_coco_masks_u8(C.byref(desc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(device)), lib)
    return DeviceMasks(miss, tables.offsets, tables.sizes, every, keep=(pinned, dev_tables))
