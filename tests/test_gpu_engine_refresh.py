"""GPU: og_fold_bn_w16 (csrc/fold.hip) through the C ABI bit for bit against the numpy restatement of the header's rule
(tests/engine_refresh_common.py) on a table of directed layers; InferenceEngine.refresh on graph engines -- same addresses, the
buffers and the replayed outputs of an engine built afresh, nothing allocated for good, two shapes behind one call.  The modules
live on the CPU (the engines built afresh fold there, the refreshed ones on the device through temporaries) or on the device in
channels-last (the parameters themselves are the kernel's sources)."""
import numpy as np
import pytest
import torch

import engine_refresh_common as rc
from offsetguided_amd import _lib, models
from offsetguided_amd.models import engine as eng_mod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests selected but no HIP device is visible')
    _lib.load()
    return torch.device('cuda:0')


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
# cout, cin, k, channels-last source, BN, bias, weight offset (floats past a 16-byte boundary), dst offset (halfs), partner row, what
ROWS = [
    (8, 3, 7, False, True, False, 0, 0, -1, 'plain'),              # stem-like: odd Cin, scalar stores
    (128, 3, 7, False, True, False, 1, 0, -1, 'plain'),            # the stem, weights 4 bytes off
    (17, 256, 1, False, False, True, 0, 0, -1, 'plain'),           # heads: no BN, bias
    (38, 256, 1, True, False, True, 0, 0, -1, 'plain'),
    (64, 64, 3, False, True, True, 2, 1, -1, 'plain'),             # 8 bytes off, a destination off its 16-byte boundary, ragged slab
    (128, 64, 3, True, True, False, 3, 0, -1, 'plain'),            # channels-last source, 12 bytes off
    (384, 256, 3, False, True, False, 0, 0, 7, 'plain'),           # junction: + the folded bias of row 7
    (384, 64, 1, False, True, True, 0, 0, -1, 'plain'),
    (64, 64, 1, False, True, True, 0, 0, -1, 'range'),             # scales that send fp16 to inf, into its subnormals and below
    (64, 256, 3, True, True, False, 0, 0, -1, 'zeros'),            # gamma = 0, sigma^2 = 0
    (8, 1024, 3, True, True, True, 1, 0, -1, 'plain'),             # 9216 values per output channel: two passes through LDS
    (8, 1000, 3, False, True, True, 0, 0, -1, 'plain'),            # OIHW in two passes (896 + 104 channels)
    (8, 8, 5, False, True, True, 0, 0, -1, 'plain'),               # a tap count without a specialised path
    (64, 64, 3, False, False, False, 0, 0, -1, 'plain'),           # neither BN nor bias: w' = w, b' = 0
]

def _row_data(spec, seed):
    cout, cin, k, cl, bn, bias, w_off, d_off, partner, what = spec
    rs = np.random.RandomState(seed)
    f = np.float32
    w = rs.randn(cout, cin, k, k).astype(f)
    b = rs.randn(cout).astype(f) if bias else None
    stats = None
    if bn:
        gamma = (10.0 ** rs.uniform(-3, 3, cout) * rs.choice([-1.0, 1.0], cout)).astype(f)
        var = (10.0 ** rs.uniform(-6, 2, cout)).astype(f)
        if what == 'zeros':
            gamma[::3] = 0.0
            var[1::4] = 0.0
        if what == 'range':
            var[:] = 1.0
            gamma[:] = (10.0 ** np.linspace(-39, 7, cout)).astype(f)     # fp32 subnormal gammas up to products beyond fp16's range
        stats = (gamma, rs.randn(cout).astype(f), rs.randn(cout).astype(f), var, 1e-3 if what == 'zeros' else 1e-5)
    return w, b, stats


def _place(values, off, dev):
    """(buffer, view): a device copy of `values` (bytes) whose first element sits `off` elements past a 16-byte boundary, inside a
    buffer of 0x77 bytes."""
    values = np.ascontiguousarray(values)
    start = 32 + off * values.itemsize
    base = torch.full((values.nbytes + 80,), 0x77, dtype=torch.uint8, device=dev)
    view = base[start:start + values.nbytes]
    view.copy_(torch.from_numpy(values.reshape(-1).view(np.uint8)))
    assert view.data_ptr() % 16 == (off * values.itemsize) % 16
    return base, view


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
def test_fold_kernel_bit_for_bit(dev, dtype):
    lib = _lib.load()
    words = lib.og_fold_row_words()
    assert words == 16
    data = [_row_data(spec, 100 + i) for i, spec in enumerate(ROWS)]
    table = np.zeros((len(ROWS), words), np.int64)
    groups, keep, outs = [], [], []
    for i, (spec, (w, b, stats)) in enumerate(zip(ROWS, data)):
        cout, cin, k, cl, bn, bias, w_off, d_off, partner, what = spec
        mem = w.transpose(0, 2, 3, 1) if cl else w
        ptrs = [_place(mem, w_off, dev)]
        ptrs.append(_place(b, 1, dev) if bias else None)
        ptrs += [_place(v, j % 4, dev) for j, v in enumerate(stats[:4])] if bn else [None] * 4
        dst = [_place(np.zeros(w.size, np.int16), d_off, dev), _place(np.zeros(cout, np.float32), 0, dev),
               _place(np.zeros(cout, np.int16), 0, dev)]
        keep.append(ptrs)
        outs.append(dst)
        slab = max(1, min(cout, 16384 // (cin * k * k)))
        eps = int(np.float32(stats[4]).view(np.int32)) if bn else 0
        table[i] = [*(p[1].data_ptr() if p is not None else 0 for p in ptrs), *(d[1].data_ptr() for d in dst), cout, cin, k * k, int(cl),
                    eps, partner, slab]
        groups.append(-(-cout // slab))
    assert {int(table[i, 0]) % 16 for i in range(len(ROWS))} >= {0, 4, 8, 12}      # every offset of a weight pointer is in the table
    prefix = np.zeros(len(ROWS) + 1, np.int32)
    np.cumsum(groups, out=prefix[1:])
    raw = torch.from_numpy(np.concatenate([table.reshape(-1).view(np.uint8), prefix.view(np.uint8)])).to(dev)
    _lib.check(lib.og_fold_bn_w16(raw.data_ptr(), raw.data_ptr() + 8 * table.size, len(ROWS), int(prefix[-1]), int(dtype == torch.float16),
                                  _lib.stream_ptr(dev)), lib)
    torch.cuda.synchronize(dev)
    seen_inf = seen_sub = False
    for i, (spec, (w, b, stats), dst) in enumerate(zip(ROWS, data, outs)):
        partner = spec[8]
        other = (data[partner][1], data[partner][2]) if partner >= 0 else None
        w16, b32, b16 = rc.fold_reference(w, b, stats, dtype, other)
        got_w = dst[0][1].cpu().numpy().view(np.uint16).reshape(w16.shape)
        assert np.array_equal(got_w, w16), f'row {i} {spec}: {int((got_w != w16).sum())} weights differ'
        assert np.array_equal(dst[1][1].cpu().numpy().view(np.uint32), b32.view(np.uint32)), f'row {i} {spec}: b32'
        assert np.array_equal(dst[2][1].cpu().numpy().view(np.uint16), b16), f'row {i} {spec}: b'
        for base, view in dst:       # nothing written outside the destinations
            flat, first = base.cpu().numpy(), view.data_ptr() - base.data_ptr()
            assert (flat[:first] == 0x77).all() and (flat[first + view.numel():] == 0x77).all(), f'row {i} {spec}: guard'
        if spec[9] == 'range' and dtype == torch.float16:
            mag = w16 & 0x7fff
            seen_inf, seen_sub = bool((mag == 0x7c00).any()), bool(((mag > 0) & (mag < 0x0400)).any())
    if dtype == torch.float16:
        assert seen_inf and seen_sub       # the directed row reached both ends of fp16's range
    rc_bad = lib.og_fold_bn_w16(None, None, 1, 1, 1, None)
    assert rc_bad == _lib.OG_EINVAL and b'null table' in lib.og_last_error()


# ---- the engine ----------------------------------------------------------------------------------------------------------------
def _input(shape, dev, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _replay(engine, x):
    out = [o.clone() for o in engine.forward_raw(x)]
    torch.cuda.synchronize()
    return out


def _same_buffers(engine, fresh):
    mine, theirs = rc.persistent(engine._layers), rc.persistent(fresh._layers)
    assert list(mine) == list(theirs)
    # every kind of derived image is in the comparison: a route threshold that moves must not drop one out of it unnoticed
    for kind in ('.w_tiled', '.w_band', '.w_alt'):
        assert any(k.endswith(kind) for k in mine), kind
    assert 'stem_w' in mine and 'heads_w' in mine and 'heads_tiled.w' in mine
    for k in mine:
        assert torch.equal(mine[k], theirs[k]), k


@pytest.mark.parametrize('resident', ['cpu', 'device_cl'])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
def test_refresh_graph_engine(dev, dtype, resident):
    """resident = device_cl: the module lives on the device in channels-last, as train_dist's does -- its parameter pointers go
    straight into the fold table (channels-last rows, no temporaries) and the engine built afresh folds with torch's device ops."""
    eng_mod.invalidate_engine_cache()
    model = rc.perturb(rc.make_model(), 1)
    if resident == 'device_cl':
        model = model.to(dev).to(memory_format=torch.channels_last)
        w3 = model.basenet.pre[1].conv1.weight
        assert w3.is_cuda and not w3.is_contiguous() and w3.is_contiguous(memory_format=torch.channels_last)
    engine = models.InferenceEngine(model, 1, 128, 128, dtype=dtype, device=dev)
    assert engine.fused and engine._graph is not None
    x = _input(engine.shape, dev, 5)
    old = _replay(engine, x)
    ptrs = {k: t.data_ptr() for k, t in rc.persistent(engine._layers).items()}
    rc.perturb(model, 2)
    engine.refresh()
    allocated = torch.cuda.memory_allocated(dev)
    engine.refresh()
    assert torch.cuda.memory_allocated(dev) == allocated
    assert {k: t.data_ptr() for k, t in rc.persistent(engine._layers).items()} == ptrs
    assert models.InferenceEngine(model, 1, 128, 128, dtype=dtype, device=dev, use_graph=False)._layers is engine._layers
    eng_mod.invalidate_engine_cache()
    fresh = models.InferenceEngine(model, 1, 128, 128, dtype=dtype, device=dev)
    assert fresh._layers is not engine._layers
    _same_buffers(engine, fresh)
    new, new_fresh = _replay(engine, x), _replay(fresh, x)
    assert all(bool(torch.isfinite(o).all()) for o in new)
    assert all(torch.equal(a, b) for a, b in zip(new, new_fresh))
    assert not any(torch.equal(a, b) for a, b in zip(new, old))


def test_two_shapes_share_one_refresh(dev):
    eng_mod.invalidate_engine_cache()
    model = rc.perturb(rc.make_model(), 1)
    square = models.InferenceEngine(model, 1, 128, 128, device=dev)
    wide = models.InferenceEngine(model, 1, 128, 256, device=dev, like=square)
    assert wide._layers is square._layers
    xs, xw = _input(square.shape, dev, 6), _input(wide.shape, dev, 7)
    old = _replay(square, xs) + _replay(wide, xw)
    rc.perturb(model, 3)
    wide.refresh()
    eng_mod.invalidate_engine_cache()
    fresh_square = models.InferenceEngine(model, 1, 128, 128, device=dev)
    fresh_wide = models.InferenceEngine(model, 1, 128, 256, device=dev, like=fresh_square)
    _same_buffers(square, fresh_wide)
    new = _replay(square, xs) + _replay(wide, xw)
    assert all(torch.equal(a, b) for a, b in zip(new, _replay(fresh_square, xs) + _replay(fresh_wide, xw)))
    assert not any(torch.equal(a, b) for a, b in zip(new, old))
