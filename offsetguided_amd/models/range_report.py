"""Range report: what the engine's 16-bit type does to weights and activations, counted on the device (include/og_decoder.h, "range
report"; csrc/range.hip).  A stats row is nine int64 words -- n, nan, inf, over, zero, flush, sub, max, min -- that every launch
accumulates into.  range_stats queues ONE launch over a list of tensors (the table is packed and uploaded by _table.py) and does
not wait; probe queues one launch on one tensor with its address as a kernel argument (the form a graph
capture needs); decode is the one place that reads anything back."""
import numpy as np
import torch

from .. import _lib, _table

WORDS = 9
NAMES = ('n', 'nan', 'inf', 'over', 'zero', 'flush', 'sub', 'max', 'min')
TYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
PROBE_MAX_WG = 1024      # workgroups of one tensor at most: beyond that each strides over several chunks (one set of atomics per workgroup)
_F32_INF = 0x7f800000
_pool = _table.Pool()


def _target(dtype):
    if dtype not in (torch.float16, torch.bfloat16):
        raise _lib.OgError(f'range report: the target type must be torch.float16 or torch.bfloat16, got {dtype}')
    return TYPE_CODE[dtype]


def _source(t, target_dtype, what):
    """The type code of a tensor the kernel can read as one dense run: on a device, fp32 or the target type, contiguous in memory in
    NCHW or channels-last order (the nine words do not depend on the order of the elements)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.OgError(f'range report: {what} must be a tensor on a HIP device (offsetguided_amd has no CPU path)')
    if t.dtype != torch.float32 and t.dtype != target_dtype:
        err = _lib.OgError(f'range report: {what} is {t.dtype}; the source must be torch.float32 or the target type {target_dtype}')
        err.code = _lib.OG_EINVAL
        raise err
    if not (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
        raise ValueError(f'range report: {what} (shape {tuple(t.shape)}, strides {t.stride()}) is not one dense run of memory')
    return TYPE_CODE[t.dtype]


def range_stats(tensors, target_dtype, rows=None, out=None):
    """Accumulate the nine words of every tensor of `tensors` into row rows[i] (default: i) of a device int64 (R, 9) tensor: `out`
    (updated in place) or a new one of zeros with max(rows) + 1 rows.  Several tensors may share a row.  One table copy and ONE
    og_range_stats launch on the current stream; never waits for the device."""
    tensors = list(tensors)
    target = _target(target_dtype)
    rows = list(range(len(tensors))) if rows is None else [int(r) for r in rows]
    if len(rows) != len(tensors):
        raise ValueError(f'range_stats: {len(tensors)} tensors but {len(rows)} rows')
    if not tensors:
        if out is None:
            raise ValueError('range_stats: no tensors and no `out` to tell the device from')
        return out
    dev = tensors[0].device
    codes = [_source(t, target_dtype, f'tensor {i}') for i, t in enumerate(tensors)]
    if any(t.device != dev for t in tensors):
        raise ValueError('range_stats: the tensors are on different devices')
    n_stats = max(rows) + 1
    if min(rows) < 0:
        raise ValueError('range_stats: negative stats row')
    lib = _lib.load()
    with torch.cuda.device(dev):
        if out is None:
            out = torch.zeros((n_stats, WORDS), dtype=torch.int64, device=dev)
        if out.dtype != torch.int64 or out.device != dev or out.dim() != 2 or out.shape[1] != WORDS or out.shape[0] < n_stats or not out.is_contiguous():
            raise ValueError(f'range_stats: `out` must be a contiguous int64 ({n_stats}+, {WORDS}) tensor on {dev}')
        chunk = lib.og_range_chunk_elems()
        table = np.zeros((len(tensors), 4), np.int64)
        groups = np.zeros(len(tensors), np.int64)
        for i, (t, code, r) in enumerate(zip(tensors, codes, rows)):
            table[i] = [t.data_ptr(), t.numel(), code, r]
            groups[i] = min(-(-t.numel() // chunk), PROBE_MAX_WG)
        raw, prefix, prefix_at = _table.pack(table, groups)
        dev_table = _table.upload(raw, dev, _pool)       # a new tensor, stream-ordered: free to go once the launch is queued
        at = dev_table.data_ptr()
        _lib.check(lib.og_range_stats(at, at + prefix_at, len(tensors), int(prefix[-1]), target, _lib.ptr(out),
                                      _lib.stream_ptr(dev)), lib)
    return out


def probe(t, target_dtype, stats, row):
    """Accumulate the nine words of ONE tensor into stats[row] with one og_range_probe launch on the current stream (pointer and size
    are kernel arguments: capturable into a graph whose tensors sit elsewhere than the warm-up's).  Never waits."""
    code = _source(t, target_dtype, 'the probed tensor')
    lib = _lib.load()
    _lib.check(lib.og_range_probe(_lib.ptr(t), t.numel(), code, _target(target_dtype), stats.data_ptr() + 8 * WORDS * row,
                                  _lib.stream_ptr(t.device)), lib)


def combine(parts):
    """Stats tensors of one shape (any device) -> their combination on the CPU: words 0..6 summed, words 7 and 8 maxima."""
    parts = [p.cpu() for p in parts]
    both = torch.stack(parts)
    return torch.cat([both[..., :7].sum(0), both[..., 7:].max(0).values], -1)


def _f32(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def decode(stats):
    """An (R, 9) stats tensor (or one row) -> a list of R dicts with the names of the header; `max` and `min` as floats: the largest
    and the smallest non-zero finite magnitude seen, 0.0 where none was.  Waits for the device (the one place that does)."""
    rows = stats.detach().cpu().reshape(-1, WORDS).tolist()
    out = []
    for r in rows:
        d = dict(zip(NAMES[:7], (int(v) for v in r[:7])))
        d['max'] = _f32(int(r[7]))
        d['min'] = _f32(_F32_INF - int(r[8])) if r[8] else 0.0
        out.append(d)
    return out
