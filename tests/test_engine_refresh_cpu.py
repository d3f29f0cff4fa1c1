"""CPU: the bookkeeping of InferenceEngine.refresh on the fp32 torch path (same buffers, new contents, the cache entry moved), the
numpy restatement of the fold rule against models.engine._fold + cast bit for bit, and SyncBatchNorm folded like BatchNorm2d."""
import numpy as np
import pytest
import torch

import engine_refresh_common as rc
from offsetguided_amd import models
from offsetguided_amd.models import engine as eng_mod

CPU = torch.device('cpu')


# ---- the rule ----------------------------------------------------------------------------------------------------------------
LAYERS = {'1x1': (24, 16, 1), '3x3': (16, 8, 3), 'stem7x7': (8, 3, 7)}


def _layer(kind, bn, bias, channels_last, seed):
    cout, cin, k = LAYERS[kind]
    g = torch.Generator().manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, k, bias=bias)
    norm = torch.nn.BatchNorm2d(cout) if bn else None
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        if bias:
            conv.bias.copy_(torch.randn(cout, generator=g))
        if bn:
            norm.weight.copy_(10.0 ** (torch.rand(cout, generator=g) * 6 - 3))
            norm.weight[1] = 0.0
            norm.running_var.copy_(10.0 ** (torch.rand(cout, generator=g) * 8 - 6))
            norm.running_var[2] = 0.0
            norm.running_mean.copy_(torch.randn(cout, generator=g))
            norm.bias.copy_(torch.randn(cout, generator=g))
    if channels_last:
        conv = conv.to(memory_format=torch.channels_last)
    return conv, norm


def _np(t):
    return None if t is None else t.detach().numpy()


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['f16', 'bf16'])
@pytest.mark.parametrize('channels_last', [False, True], ids=['oihw', 'cl'])
@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('bn', [False, True], ids=['nobn', 'bn'])
@pytest.mark.parametrize('kind', list(LAYERS))
def test_restatement_equals_fold_and_cast(kind, bn, bias, channels_last, dtype):
    conv, norm = _layer(kind, bn, bias, channels_last, 11)
    w, b = eng_mod._fold(conv, norm)
    w_t = w.to(dtype).contiguous(memory_format=torch.channels_last)
    stats = (_np(norm.weight), _np(norm.bias), _np(norm.running_mean), _np(norm.running_var), norm.eps) if bn else None
    w16, b32, b16 = rc.fold_reference(_np(conv.weight), _np(conv.bias), stats, dtype)
    assert np.array_equal(rc.bits16(w_t.permute(0, 2, 3, 1)), w16)
    assert np.array_equal(b.float().numpy().view(np.uint32), b32.view(np.uint32))
    assert np.array_equal(rc.bits16(b.to(dtype)), b16)


# ---- the engine ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    return rc.perturb(rc.make_model(), 1)


def _stats(bn):
    return None if bn is None else (_np(bn.weight), _np(bn.bias), _np(bn.running_mean), _np(bn.running_var), bn.eps)


def test_restatement_equals_the_bundle_of_the_whole_model(model):
    """Every layer of a built bundle, junction biases included, against the restatement: ~50 000 channels.  (torch's own fp32 sqrt is
    not correctly rounded -- on the CPU one result in 160 misses its last bit -- so _fold takes root and quotient in double; a layer
    of a few channels does not see the difference, this model does.)"""
    layers = models.engine._Layers(model, torch.float16, CPU, 1, False)
    mods = dict(model.named_modules())
    n = 0
    for c, partner in layers._convs():
        conv, bn = mods[c.name], mods[c.bn_name] if c.bn_name else None
        other = None
        if partner is not None:
            other = (_np(mods[partner.name].bias), _stats(mods[partner.bn_name] if partner.bn_name else None))
        w16, b32, b16 = rc.fold_reference(_np(conv.weight), _np(conv.bias), _stats(bn), torch.float16, other)
        assert np.array_equal(rc.bits16(c.w.permute(0, 2, 3, 1)), w16), c.name
        assert np.array_equal(c.b32.numpy().view(np.uint32), b32.view(np.uint32)), c.name
        assert np.array_equal(rc.bits16(c.b), b16), c.name
        n += len(b32)
    assert n > 40000


def _engine(model, h=128, w=128, **kw):
    return models.InferenceEngine(model, 1, h, w, dtype=torch.float32, device='cpu', use_graph=False, **kw)


def _forward(engine, seed=5):
    x = torch.randn(engine.shape, generator=torch.Generator().manual_seed(seed))
    return [o.clone() for o in engine.forward_raw(x)]


def test_refresh_in_place_equals_a_fresh_engine_and_moves_the_cache(model):
    eng_mod.invalidate_engine_cache()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    engine = _engine(model)
    wide = _engine(model, 128, 256, like=engine)            # another shape on the same bundle
    assert wide._layers is engine._layers
    old, old_wide = _forward(engine), _forward(wide)
    tensors = rc.persistent(engine._layers)
    ptrs = {k: t.data_ptr() for k, t in tensors.items()}
    rc.perturb(model, 2)
    assert engine.refresh() is engine
    assert {k: t.data_ptr() for k, t in rc.persistent(engine._layers).items()} == ptrs
    # a new engine on the same module finds the refreshed bundle; one built from scratch computes the same
    again = _engine(model)
    assert again._layers is engine._layers
    eng_mod.invalidate_engine_cache()
    fresh = _engine(model)
    assert fresh._layers is not engine._layers
    for (k, t), (k2, t2) in zip(tensors.items(), rc.persistent(fresh._layers).items()):
        assert k == k2 and torch.equal(t, t2), k
    new, new_fresh = _forward(engine), _forward(fresh)
    assert all(torch.isfinite(o).all() for o in new)
    assert all(torch.equal(a, b) for a, b in zip(new, new_fresh))
    assert not any(torch.equal(a, b) for a, b in zip(new, old))
    # the engine of the other shape changed with the same call
    new_wide, wide_fresh = _forward(wide), _forward(_engine(model, 128, 256, like=fresh))
    assert all(torch.equal(a, b) for a, b in zip(new_wide, wide_fresh))
    assert not any(torch.equal(a, b) for a, b in zip(new_wide, old_wide))
    # the module put back to the weights the bundle was first built from is not served the refreshed bundle
    eng_mod.invalidate_engine_cache()
    engine.refresh()
    assert _engine(model)._layers is engine._layers
    model.load_state_dict(before)
    back = _engine(model)
    assert back._layers is not engine._layers
    assert all(torch.equal(a, b) for a, b in zip(_forward(back), old))


def test_refresh_takes_another_module_of_the_same_shapes(model):
    eng_mod.invalidate_engine_cache()
    engine = _engine(model)
    # the bundle owns its storage: the heads (no BatchNorm, fp32 on the same device) would otherwise BE the module's parameters
    owned = {t.data_ptr() for t in rc.persistent(engine._layers).values()}
    assert not owned & {t.data_ptr() for t in list(model.parameters()) + list(model.buffers())}
    before = {k: v.clone() for k, v in model.state_dict().items()}
    other = rc.perturb(rc.make_model(), 3)
    engine.refresh(other)
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), 'refresh(other) wrote into the module the engine was built from'
    first = engine._layers._finalizer
    engine.refresh(other)
    assert not first.alive and engine._layers._finalizer.alive      # the cache entry's finalizer is replaced, not added to
    assert _engine(other)._layers is engine._layers
    assert _engine(model)._layers is not engine._layers          # `model` is no longer what the bundle holds
    fresh = rc.persistent(models.engine._Layers(other, torch.float32, CPU, engine.stage, False))
    for (k, t), (k2, t2) in zip(rc.persistent(engine._layers).items(), fresh.items()):
        assert k == k2 and torch.equal(t, t2), k
    small = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3))
    with pytest.raises(ValueError, match='refresh'):
        engine.refresh(small)


def test_sync_batchnorm_is_folded(model):
    import copy
    plain = rc.persistent(models.engine._Layers(model, torch.float32, CPU, 1, False))
    synced = torch.nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(model))
    assert any(isinstance(m, torch.nn.SyncBatchNorm) for m in synced.modules())
    layers = models.engine._Layers(synced, torch.float32, CPU, 1, False)
    folded = rc.persistent(layers)
    assert len(folded) == len(plain)
    for (k, t), (k2, t2) in zip(plain.items(), folded.items()):
        assert k == k2 and torch.equal(t, t2), k
    # ... and differs from the unfolded convolution weights: the BN was not skipped
    first = next(iter(layers._convs()))[0]
    assert not torch.equal(first.w, synced.basenet.pre[0].conv.weight.detach())
    # refresh folds it as well
    rc.perturb(synced, 4)
    layers.refresh(synced)
    again = rc.persistent(models.engine._Layers(synced, torch.float32, CPU, 1, False))
    for (k, t), (k2, t2) in zip(rc.persistent(layers).items(), again.items()):
        assert k == k2 and torch.equal(t, t2), k
