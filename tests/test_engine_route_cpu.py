"""Which kernel models/engine.py picks for a layer and for a residual block, as a table: _Conv.route and _Residual.route take shapes
only, so the table needs no GPU (the library is loaded for its host-side *_supported queries).  The rows were derived by hand from
the cascade and the C predicates (tiled_kind, og_conv3x3s2_tiled_supported, band_plan); the first group is what ROUTES of
tests/test_gpu_engine_exact.py meets on the device.  Layers and blocks are built on the CPU with fused=True: the constructors only fold
weights."""
import os
import re

import pytest
import torch

from offsetguided_amd import _lib
from offsetguided_amd.models import engine as E
from offsetguided_amd.models.hourglass_104 import ConvBlock, Residual

F16 = torch.float16
DEFAULTS = dict(CONV_TILED=7, CONV_UP2=1, CONV_BAND_MAX_PIXELS=1024, CONV_TILED_MIN_PIXELS=2048, CONV3X3_MAX_PIXELS=8192,
                CONV_S2_MAX_PIXELS=8192, CONV_SPLITK_LAST_RESORT=1 << 17, CONV_PW_MIN_PIXELS=1024, _WHATIF=set())


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    _lib.load()
    for k, v in DEFAULTS.items():
        monkeypatch.setattr(E, k, v)
    return monkeypatch


_convs, _blocks = {}, {}


def _conv(cin, cout, stride):
    if (cin, cout, stride) not in _convs:
        _convs[cin, cout, stride] = E._Conv(torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False), None, True, F16, True)
    return _convs[cin, cout, stride]


def _block(cin, cout, stride=1):
    if (cin, cout, stride) not in _blocks:
        _blocks[cin, cout, stride] = E._Residual(Residual(cin, cout, stride), F16, True)
    return _blocks[cin, cout, stride]


def _route(n, h, w, cin, cout, stride, **kw):
    return _conv(cin, cout, stride).route((n, cin, h, w), F16, kw.pop('on_gpu', True), **kw)


#        N, Hin, Win, Cin, Cout, stride, route
LAYERS = [(1, 80, 48, 256, 256, 1, 'tiled'),
          (1, 40, 40, 256, 256, 1, 'splitk'),         # 1600 pixels < CONV_TILED_MIN_PIXELS
          (2, 10, 10, 384, 384, 1, 'band'),
          (2, 5, 5, 512, 512, 1, 'band'),
          (2, 10, 10, 384, 512, 2, 'band'),
          (1, 224, 160, 256, 256, 2, 'tiled_s2'),     # 8960 output pixels
          (8, 40, 40, 384, 384, 2, 'splitk'),         # 3200 <= CONV_S2_MAX_PIXELS
          (8, 20, 20, 384, 384, 1, 'tiled'),          # tile kind 3
          (1, 100, 100, 256, 256, 1, 'splitk'),       # last resort: no tile shape, 10 000 <= 131 072
          (8, 200, 200, 256, 256, 1, 'torch'),
          (1, 160, 160, 64, 64, 1, 'splitk'),         # last resort: Cout % 128 != 0
          (1, 64, 64, 3, 128, 1, 'torch'),
          (1, 64, 64, 128, 17, 1, 'torch')]
BAND = [r for r in LAYERS if r[-1] == 'band']


@pytest.mark.parametrize("row", LAYERS, ids=lambda r: 'x'.join(map(str, r[:6])))
def test_layer_routes(row):
    assert _route(*row[:6]) == row[6]
    assert _route(*row[:6], on_gpu=False) not in ('band', 'up2')
    assert _route(*row[:6], merge=True) == ('up2' if row[6] == 'tiled' else row[6])


def test_a_layer_that_is_no_3x3_of_the_kernels_is_torch():
    c = E._Conv(torch.nn.Conv2d(256, 256, 1), None, True, F16, True)
    assert not c.hip3x3 and c.route((1, 256, 80, 48), F16, True) == 'torch'
    c = E._Conv(torch.nn.Conv2d(256, 256, 3, padding=1), None, True, torch.float32, False)       # the fp32 checking path
    assert c.route((1, 256, 80, 48), torch.float32, False) == 'torch'


def test_block_routes():
    assert _block(384, 256).route((1, 384, 40, 40), (1, 256, 40, 40), F16, True) == (None, 'splitk+proj')
    assert _block(128, 256, 2).route((1, 128, 64, 64), (1, 256, 32, 32), F16, True) == (None, 'band+proj')
    down = _block(256, 256, 2)
    assert down.skip is not None and down.route((1, 256, 224, 160), (1, 256, 112, 80), F16, True) == ('pointwise', 'tiled')
    same = _block(256, 256)
    assert same.skip is None
    assert same.route((1, 256, 80, 48), (1, 256, 80, 48), F16, True, merge=True) == (None, 'up2')
    assert same.route((1, 256, 80, 48), (1, 256, 80, 48), F16, True) == (None, 'tiled')
    assert same.route((2, 256, 10, 10), (2, 256, 10, 10), F16, True, merge=True) == (None, 'band')
    # a merge goes to the block's conv2 even where the projection is computed apart
    assert down.route((1, 256, 224, 160), (1, 256, 112, 80), F16, True, merge=True) == ('pointwise', 'up2')
    # not on the device: nothing that needs it
    assert down.route((1, 256, 224, 160), (1, 256, 112, 80), F16, False, merge=True) == ('torch', 'tiled')
    assert down.route((1, 256, 224, 160), (1, 256, 112, 80), F16, True, channels_last=False) == ('torch', 'tiled')


def test_band_knob(knobs):
    knobs.setattr(E, 'CONV_BAND_MAX_PIXELS', 0)
    for row in BAND:
        assert _route(*row[:6]) == 'splitk'
    assert _block(128, 256, 2).route((1, 128, 64, 64), (1, 256, 32, 32), F16, True) == (None, 'splitk+proj')


def test_up2_knob(knobs):
    knobs.setattr(E, 'CONV_UP2', 0)
    assert _route(1, 80, 48, 256, 256, 1, merge=True) == 'tiled'
    assert _block(256, 256).route((1, 256, 80, 48), (1, 256, 80, 48), F16, True, merge=True) == (None, 'tiled')


def test_tiled_knob(knobs):
    """Without the tiled kernels a 3x3 layer is the split-K kernel's up to CONV3X3_MAX_PIXELS by preference, up to
    CONV_SPLITK_LAST_RESORT for want of another, and torch's beyond."""
    knobs.setattr(E, 'CONV_TILED', 0)
    assert _route(1, 160, 160, 256, 256, 1) == 'splitk' and _route(1, 224, 160, 256, 256, 2) == 'splitk'
    knobs.setattr(E, 'CONV_SPLITK_LAST_RESORT', 0)
    assert _route(1, 80, 48, 256, 256, 1) == 'splitk'            # 3840 pixels <= CONV3X3_MAX_PIXELS
    assert _route(1, 160, 160, 256, 256, 1) == 'torch' and _route(1, 224, 160, 256, 256, 2) == 'torch'
    knobs.setattr(E, 'CONV3X3_MAX_PIXELS', 2048)
    assert _route(1, 80, 48, 256, 256, 1) == 'torch'


def test_pointwise_knob(knobs):
    knobs.setattr(E, 'CONV_TILED', 3)
    assert _block(256, 256, 2).route((1, 256, 224, 160), (1, 256, 112, 80), F16, True) == ('torch', 'tiled')
    assert not E._heads_tiled_ok(256, 2)


def test_stride2_tiled_needs_a_channels_last_input():
    assert _route(1, 224, 160, 256, 256, 2, channels_last=False) == 'splitk'


def test_whatif_keeps_the_layers_off_the_fused_routes(knobs):
    knobs.setattr(E, '_WHATIF', {'c80'})
    assert _route(2, 10, 10, 384, 384, 1) == 'splitk' and _route(1, 80, 48, 256, 256, 1, merge=True) == 'tiled'
    assert _block(384, 256).route((1, 384, 40, 40), (1, 256, 40, 40), F16, True) == ('torch', 'splitk')


def test_junction_and_heads():
    a = E._Conv(torch.nn.Conv2d(256, 256, 1), None, True, F16, True)
    assert a.pointwise_ok((1, 256, 64, 64), True, x2_shape=(1, 256, 64, 64))
    assert not a.pointwise_ok((1, 256, 64, 64), True, x2_shape=(1, 256, 32, 32))
    assert not a.pointwise_ok((1, 256, 16, 16), True) and not a.pointwise_ok((1, 256, 64, 64), False)      # 256 pixels; not on the GPU
    assert not a.pointwise_ok((1, 256, 64, 64), True, channels_last=False)
    assert E._heads_tiled_ok(256, 2) and E._heads_tiled_ok(256, 4) and not E._heads_tiled_ok(256, 5)
    assert not E._heads_tiled_ok(96, 2) and not E._heads_tiled_ok(256, 2, channels_last=False)


def test_the_library_is_asked_in_one_place():
    src = open(os.path.join(os.path.dirname(E.__file__), 'engine.py')).read()
    for name in ('og_conv_band_supported', 'og_conv3x3_tiled_supported', 'og_conv3x3s2_tiled_supported'):
        assert len(re.findall(name + r'\b', src)) == 1, name


def test_a_failed_build_leaves_the_thread_clean(knobs):
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.basenet = torch.nn.Module()
            self.basenet.pre = torch.nn.ModuleList([ConvBlock(7, 3, 128, stride=2), Residual(128, 256, stride=2)])
    seen = []

    def boom(*a):
        seen.append((E._issuer.build_device, E._issuer.names is not None))
        raise RuntimeError('cannot fold')
    knobs.setattr(E, '_Residual', boom)
    with pytest.raises(RuntimeError, match='cannot fold'):
        E._Layers(Net(), F16, torch.device('cpu'), 0, False)
    assert seen == [(torch.device('cpu'), True)]
    assert E._issuer.build_device is None and E._issuer.names is None
