"""Tensor tables: the host side of the one-launch-over-many-tensors kernels (csrc/table.h; optim.py, models/fold.py,
models/range_report.py).  A table is the rows (int64 words: addresses, sizes, flags) followed by an int32 running sum of the rows'
workgroup counts.  pack() builds its bytes (pure numpy), upload() sends them through pinned memory with one copy that never waits."""
import numpy as np
import torch


class _Slot:
    """One pinned staging area; `event` is recorded behind the copy that reads it."""

    def __init__(self, nbytes):
        self.buf = torch.empty(max(nbytes, 4096), dtype=torch.uint8).pin_memory()
        self.event = None

    def free(self):
        # the non-blocking copy reads the pinned bytes when the stream gets there, not when it is queued: the slot may be written again
        # only once the event behind that copy has completed (query() asks, it does not wait)
        return self.event is None or self.event.query()


class Pool:
    """The pinned slots of one owner of tables (an optimizer, an engine's weight bundle, the range report)."""

    def __init__(self):
        self._slots = []

    def take(self, nbytes):
        """A free slot of at least nbytes; a new one, with room for a table twice as large, when every fitting one is still being read."""
        slot = next((s for s in self._slots if s.buf.numel() >= nbytes and s.free()), None)
        if slot is None:
            slot = _Slot(2 * nbytes)
            self._slots.append(slot)
        return slot


def pack(table, counts, extra=None):
    """table: int64 (n_rows, words); counts: the workgroups of every row (0: the kernel passes the row over); extra: int64 words that
    travel between the rows and the prefix (a column a kernel takes as a table of its own: at byte 8 * table.size of raw).
    -> (raw, prefix, offset): the table's bytes (uint8: the rows, the extra words, then the prefix), the int32 prefix [0, counts[0],
    counts[0] + counts[1], ...] and the byte offset of the prefix inside raw (a multiple of 8: whole int64 words lie before it)."""
    table = np.ascontiguousarray(table, dtype=np.int64)
    prefix = np.zeros(table.shape[0] + 1, dtype=np.int32)
    np.cumsum(counts, out=prefix[1:])
    words = [table.reshape(-1)] if extra is None else [table.reshape(-1), np.ascontiguousarray(extra, dtype=np.int64).reshape(-1)]
    return np.concatenate([w.view(np.uint8) for w in words] + [prefix.view(np.uint8)]), prefix, 8 * sum(w.size for w in words)


def upload(raw, device, pool, out=None):
    """Queue ONE non-blocking copy of pack()'s bytes to `device` on its current stream -> the uint8 device tensor that holds them:
    `out` (the tensor of an earlier upload) when it has the size, else a new one.  Never waits for the device."""
    slot = pool.take(raw.size)
    slot.buf[:raw.size].copy_(torch.from_numpy(raw))
    if out is None or out.numel() != raw.size:
        out = torch.empty(raw.size, dtype=torch.uint8, device=device)
    out.copy_(slot.buf[:raw.size], non_blocking=True)
    slot.event = torch.cuda.Event()
    slot.event.record(torch.cuda.current_stream(device))
    return out
