"""CPU-only: og_topk_workspace_bytes and og_generate_limbs_workspace_bytes (pure host arithmetic, csrc/nms_topk.hip) return what the
build that recorded tests/golden/k1_workspace_bytes.json returned, so that a workspace sized by an earlier build keeps working.

The grid: W % 4 != 0 and W % 4 == 0 on both sides of a wave-count step (62 / 63 strips, W / 4 = 58 / 59), H = 1, 79, 80, 81, 640 and
one H > 64 * 80, k = 1, 32, 226, 227, 512, and the shapes that return 0 (too wide for 16 waves, k too large for the LDS)."""
import json
import os

import pytest

from offsetguided_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'k1_workspace_bytes.json')


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_grid_covers_the_steps(golden):
    rows = golden['topk']
    assert {62, 63, 248, 252, 232, 236} <= {r[2] for r in rows}
    assert {1, 79, 80, 81, 640} <= {r[1] for r in rows} and max(r[1] for r in rows) > 64 * 80
    assert {1, 32, 226, 227, 512} <= {r[3] for r in rows}
    assert any(r[2] == 3972 and r[3] == 1 and r[4] == 0 for r in rows)          # too wide
    assert any(r[2] == 64 * 4 - 8 and r[3] == 2000 and r[4] == 0 for r in rows)  # one wave, k too large for the LDS
    assert sum(r[4] > 0 for r in rows) > len(rows) // 2


def test_topk_workspace_bytes(golden):
    lib = _lib.load()
    got = [lib.og_topk_workspace_bytes(p, h, w, k) for p, h, w, k, _ in golden['topk']]
    assert got == [r[4] for r in golden['topk']]


def test_generate_limbs_workspace_bytes(golden):
    lib = _lib.load()
    got = [lib.og_generate_limbs_workspace_bytes(n, c, h, w, k) for n, c, h, w, k, _ in golden['limbs']]
    assert got == [r[5] for r in golden['limbs']]
