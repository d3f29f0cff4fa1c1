"""Optional heatmap-weighted offset refinement (reference decoder/offset.py:8-43).

Off by default in the reference (`scored_off=False`, decoder/factory.py:52; evaluate.py never enables it).  On the device it is HIP
like every other decoder stage: `PostProcess(scored_off=True)` refines every offset tap INSIDE the pairing kernel
(og_generate_limbs_f32 with score_ksize in its descriptor: the refined tensor is never built), and the public function
`scored_offset` on device tensors is one launch of og_scored_offset_f32 (csrc/scored_offset.hip).  Both are bit-identical to the
torch-CPU formulation below, which stays for CPU tensors only: tests/test_oracle_golden.py and tools/gen_golden.py use it as the
witness of equality with the imported reference.  It is not a fallback of the decoder -- PostProcess still refuses CPU features.
Differences from the reference: works for batch size 1 (the reference's `.squeeze()` at :31 breaks there).
"""
import torch
import torch.nn.functional as F

from .. import _lib


def pack_jtypes(skeleton):
    return [a for a, _ in skeleton], [b for _, b in skeleton]


def scored_offset(hmp, off, jtypes_f, jtypes_t, kernel_size=7):
    """sum_box(hm * off) / (sum_box(hm) + 1e-6) per limb, hm = heatmap of the limb's start joint.

    Device tensors: one launch of og_scored_offset_f32 (odd kernel_size up to 7).  CPU tensors: the torch formulation, the
    reference-equality witness of the golden tests (same bit patterns: the kernel sums in avg_pool2d's CPU order)."""
    if off.is_cuda:
        return scored_offset_device(hmp, off, jtypes_f, kernel_size)
    n, _, h, w = off.shape
    pad = (kernel_size - 1) // 2
    weight = hmp[:, jtypes_f]                                   # (n, L, h, w)
    pairs = off.view(n, -1, 2, h, w)
    num = F.avg_pool2d((weight.unsqueeze(2) * pairs).view(n, -1, h, w), kernel_size, stride=1, padding=pad,
                       divisor_override=1)
    den = F.avg_pool2d(weight, kernel_size, stride=1, padding=pad, divisor_override=1)
    return (num.view(n, -1, 2, h, w) / (den.unsqueeze(2) + 1e-6)).view(n, -1, h, w)


def scored_offset_device(hmp, off, jtypes_f, kernel_size):
    """og_scored_offset_f32 on (N,C,h,w) heat maps and (N,2L,h,w) offsets -> the refined offsets, a new (N,2L,h,w) tensor."""
    hmp = _lib.require_device(hmp, 'hmps')
    off = _lib.require_device(off, 'offs')
    n, c, h, w = hmp.shape
    n_limbs = len(jtypes_f)
    assert tuple(off.shape) == (n, 2 * n_limbs, h, w), 'offsets must be (N, 2 x number of limbs, h, w) on the grid of the heat maps'
    if not all(0 <= j < c for j in jtypes_f):
        raise ValueError(f'start joints {list(jtypes_f)} do not fit {c} heat-map channels')
    dev, lib = hmp.device, _lib.load()
    out = torch.empty_like(off)
    with _lib.stage_timer('scored_offset', dev):
        _lib.check(lib.og_scored_offset_f32(_lib.ptr(hmp), _lib.ptr(off), n, c, n_limbs, h, w, _lib.ptr(_lib.int_table(jtypes_f, dev)),
                                            int(kernel_size), _lib.ptr(out), _lib.stream_ptr(dev)), lib)
    return out
