"""CPU-only: the host arithmetic of the convolution kernels (csrc/conv3x3.hip: the split-K plan and its workspace layout, the tiled
kernels' kind, K split and slab size) returns what the build that recorded tests/golden/conv_workspace_bytes.json returned
(tools/gen_golden_conv_workspace.py), so that a workspace sized by an earlier build keeps working and the engine's routing sees the
same `*_supported` answers.  Plain equality on every row.

The first test asserts that the recorded grid contains every step of that arithmetic: M = 2047 / 2048 / 2049, 1023 / 1024 tiles,
1x1 with one and two K steps, a projection K that does not divide, every (ksize, stride) and refused ones, 199 / 200 tiled work items,
chunk counts that divide and do not divide by 4 (20-wide) and 6 (40-wide), all four kinds, odd stride-2 inputs, the 40-wide stride-2
form, channel violations and the 2^30-element refusals."""
import json
import os

import pytest

from offsetguided_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_workspace_bytes.json')
FIXED = 256 + 16384 * 4      # zero page + tickets: what a plan without a K split needs


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def test_grid_covers_the_steps(golden):
    total = sum(len(v) for v in golden.values())
    assert 1000 < total <= 4000
    # ---- split-K plan
    c3 = golden['conv3x3']
    assert {2047, 2048, 2049} <= {r[0] for r in c3}
    tiles = {((r[0] + 63) // 64) * (r[2] // 64) for r in c3 if r[0] > 0 and r[1] % 64 == 0 and r[2] % 64 == 0}
    assert {1023, 1024} <= tiles
    assert any(r[0] >= 65473 and r[3] == FIXED for r in c3) and any(r[3] > FIXED for r in c3)
    c2 = golden['conv2d']
    assert {2047, 2048, 2049} <= {r[0] * r[1] * r[2] for r in c2 if r[5] == 1 and r[6] == 1}
    assert {(1, 1), (1, 2), (3, 1), (3, 2)} <= {(r[5], r[6]) for r in c2}
    assert any(r[5] not in (1, 3) and r[7] == 0 for r in c2) and any(r[6] not in (1, 2) and r[7] == 0 for r in c2)
    assert any(r[5] == 1 and r[3] == 64 and r[4] % 64 == 0 and r[0] > 0 and r[7] == 0 for r in c2)       # one K step: no plan
    assert any(r[5] == 1 and r[3] == 128 and r[7] >= FIXED for r in c2)                                   # two K steps: 3 stages
    assert any(r[3] % 64 and r[7] == 0 for r in c2) and any(r[4] % 64 and r[7] == 0 for r in c2)
    assert any(r[0] <= 0 and r[7] == 0 for r in c2)
    assert {2047, 2048, 2049} <= {r[0] * r[1] * r[2] for r in golden['conv3x3_nhw']}
    pj = golden['conv2d_proj']
    steps = lambda r: r[5] * r[5] * r[3] // 64 + r[7] // 64        # noqa: E731
    small = lambda r: r[0] * _out(r[1], r[5], r[6]) * _out(r[2], r[5], r[6])      # noqa: E731
    # a K that no admissible split divides (2 .. 6 below 2048 pixels, 3 from there), and the plan still splits
    assert any(r[7] > 0 and r[7] % 64 == 0 and small(r) < 2048 and all(steps(r) % k for k in range(2, 7)) and r[8] > FIXED for r in pj)
    assert any(r[7] > 0 and r[7] % 64 == 0 and small(r) >= 2048 and steps(r) % 3 and r[8] > FIXED for r in pj)
    assert any(r[7] % 64 and r[8] == 0 for r in pj) and any(r[7] == 0 and r[8] == 0 for r in pj)
    assert {(1, 1), (1, 2), (3, 1), (3, 2)} <= {(r[5], r[6]) for r in pj}
    # ---- tiled, stride 1: rows are [N, H, W, Cin, Cout, kind, bytes]
    td = golden['tiled']
    assert {r[5] for r in td} == {0, 1, 2, 3}
    for kind, tw, div in ((3, 20, 4), (2, 40, 6)):
        rows = [r for r in td if r[5] == kind]
        items = {r[0] * (r[1] // 4) * (r[2] // tw) * (r[4] // 128) for r in rows}
        assert {199, 200} <= items, (kind, sorted(items))
        assert any((r[3] // 32) % div == 0 and r[6] > 0 for r in rows) and any((r[3] // 32) % div and r[6] == 0 for r in rows)
        assert any((r[3] // 32) % div == 0 and r[6] == 0 for r in rows)       # 200 items and more: no split whatever the chunks
    assert any(r[3] % 64 and r[5] == 0 for r in td) and any(r[4] % 128 and r[5] == 0 for r in td)
    assert any(r[0] * r[1] * r[2] * r[3] >= 1 << 30 and r[3] % 64 == 0 and r[4] % 128 == 0 and r[1] % 16 == 0 and r[2] % 16 == 0 and r[5] == 0
               for r in td)
    assert any(r[0] * r[1] * r[2] * max(r[3], r[4]) < 1 << 30 and r[0] * r[1] * r[2] >= 63 << 16 and r[5] == 1 for r in td)
    assert any(r[0] <= 0 and r[5] == 0 for r in td)
    # ---- tiled, stride 2: rows are [N, Hin, Win, Cin, Cout, kind]
    s2 = golden['s2_tiled']
    assert {r[5] for r in s2} == {0, 1, 2}
    ok = lambda r: r[0] > 0 and r[3] % 64 == 0 and r[4] % 128 == 0      # noqa: E731
    assert any(ok(r) and r[1] % 2 and r[5] == 0 for r in s2) and any(ok(r) and r[2] % 2 and r[5] == 0 for r in s2)
    assert any(r[2] == 80 and r[1] % 4 == 0 and r[5] == 2 for r in s2) and any(ok(r) and r[2] == 80 and r[1] % 4 == 2 and r[5] == 0 for r in s2)
    assert any(r[3] % 64 and r[5] == 0 for r in s2) and any(r[3] % 64 == 0 and r[4] % 128 and r[5] == 0 for r in s2)
    assert any(ok(r) and r[0] * r[1] * r[2] * r[3] >= 1 << 30 and r[1] % 32 == 0 and r[2] % 32 == 0 and r[5] == 0 for r in s2)
    assert any(ok(r) and r[0] * r[1] * r[2] * r[3] < 1 << 30 and r[0] * r[1] * r[2] * r[4] >= 1 << 32 and r[5] == 0 for r in s2)
    assert any(ok(r) and r[0] * r[1] * r[2] >= 1 << 22 and r[5] == 1 for r in s2)


def test_conv3x3_workspace_bytes(golden):
    lib = _lib.load()
    assert [lib.og_conv3x3_workspace_bytes(*r[:3]) for r in golden['conv3x3']] == [r[3] for r in golden['conv3x3']]
    assert [lib.og_conv3x3_workspace_bytes_nhw(*r[:5]) for r in golden['conv3x3_nhw']] == [r[5] for r in golden['conv3x3_nhw']]


def test_conv2d_workspace_bytes(golden):
    lib = _lib.load()
    assert [lib.og_conv2d_workspace_bytes(*r[:7]) for r in golden['conv2d']] == [r[7] for r in golden['conv2d']]


def test_conv2d_proj_workspace_bytes(golden):
    lib = _lib.load()
    assert [lib.og_conv2d_proj_workspace_bytes(*r[:8]) for r in golden['conv2d_proj']] == [r[8] for r in golden['conv2d_proj']]


def test_conv3x3_tiled_supported_and_workspace_bytes(golden):
    lib = _lib.load()
    rows = golden['tiled']
    assert [lib.og_conv3x3_tiled_supported(*r[:5]) for r in rows] == [r[5] for r in rows]
    assert [lib.og_conv3x3_tiled_workspace_bytes(*r[:5]) for r in rows] == [r[6] for r in rows]


def test_conv3x3s2_tiled_supported(golden):
    lib = _lib.load()
    rows = golden['s2_tiled']
    assert [lib.og_conv3x3s2_tiled_supported(*r[:5]) for r in rows] == [r[5] for r in rows]
