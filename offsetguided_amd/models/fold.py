"""The HIP side of InferenceEngine.refresh: the table of og_fold_bn_w16 (include/og_decoder.h, "weight refresh"; csrc/fold.hip) for a
weight bundle (models/engine.py:_Layers) and its one launch.  The table is packed and uploaded by _table.py."""
import numpy as np
import torch

from .. import _lib, _table

SLAB_ELEMS = 16384      # weights one workgroup folds: whole output channels, at least one


def fold_bundle(layers, convs, pairs, events=None):
    """Queue ONE og_fold_bn_w16 launch on the current stream that writes w, b32 and b of every _Conv of `convs` ([(conv, partner)],
    _Layers._convs) from the modules of `pairs` ([(torch conv, BatchNorm or None)]).  Sources that are not fp32 on the bundle's device
    (a module on the CPU) go through temporaries.  events: a list that receives the (start, end) HIP timing events round the launch."""
    lib, dev, keep = _lib.load(), layers.device, []
    words = lib.og_fold_row_words()

    def src(t):
        """fp32 on the bundle's device: the tensor itself where it is that, else a temporary (alive until the launch is queued)"""
        if t is None:
            return None
        t = t.detach()
        if t.device != dev or t.dtype != torch.float32:
            t = t.to(dev, torch.float32)
        if t.dim() == 1 and not t.is_contiguous():
            t = t.contiguous()
        keep.append(t)
        return t

    index = {id(c): i for i, (c, _) in enumerate(convs)}
    table = np.zeros((len(convs), words), np.int64)
    groups = np.zeros(len(convs), np.int64)
    for i, ((c, partner), (conv, bn)) in enumerate(zip(convs, pairs)):
        w = src(conv.weight)
        channels_last = 0
        if not w.is_contiguous():
            if w.is_contiguous(memory_format=torch.channels_last):
                channels_last = 1
            else:
                w = w.contiguous()
                keep.append(w)
        cout, cin, kh, kw = w.shape
        stats = [src(bn.weight), src(bn.bias), src(bn.running_mean), src(bn.running_var)] if bn is not None else [None] * 4
        if bn is not None and any(v is None for v in stats):
            raise ValueError(f'refresh: the BatchNorm of {c.name!r} has no affine parameters or no running statistics')
        vecs = [src(conv.bias)] + stats
        assert c.w.is_contiguous(memory_format=torch.channels_last) and c.b32.is_contiguous() and c.b.is_contiguous()
        assert c.b32.numel() == cout and c.b.numel() == cout and (partner is None or partner.w.shape[0] == cout)
        slab = max(1, min(cout, SLAB_ELEMS // (cin * kh * kw)))
        eps = int(np.float32(bn.eps).view(np.int32)) if bn is not None else 0
        table[i] = [w.data_ptr(), *(v.data_ptr() if v is not None else 0 for v in vecs), c.w.data_ptr(), c.b32.data_ptr(),
                    c.b.data_ptr(), cout, cin, kh * kw, channels_last, eps, index[id(partner)] if partner is not None else -1, slab]
        groups[i] = -(-cout // slab)
    raw, prefix, prefix_at = _table.pack(table, groups)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        layers._fold_table = _table.upload(raw, dev, layers._fold_pool, out=layers._fold_table)
        rows = layers._fold_table.data_ptr()
        if events is not None:
            events.append((_lib.TimingEvent(), _lib.TimingEvent()))
            events[-1][0].record(stream)
        _lib.check(lib.og_fold_bn_w16(rows, rows + prefix_at, len(convs), int(prefix[-1]), int(layers.dtype == torch.float16),
                                      _lib.stream_ptr(dev)), lib)
        if events is not None:
            events[-1][1].record(stream)
