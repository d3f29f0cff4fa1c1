#!/usr/bin/env python3
"""Record tests/golden/conv_workspace_bytes.json: what the built library returns for the host arithmetic of the convolution kernels
(csrc/conv3x3.hip: make_plan / ws_layout, the tiled kernels' kind, K split and slab size) on a directed grid of shapes.
tests/test_conv_workspace_cpu.py holds every later build to these values by plain equality, so that a workspace sized by an earlier
build keeps working and a `*_supported` answer never changes under the engine's routing.

Run it on the commit whose arithmetic is to be kept, BEFORE a change to those functions.  No GPU is needed.
usage: python tools/gen_golden_conv_workspace.py
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_workspace_bytes.json')

# ---- the split-K kernel's plan -------------------------------------------------------------------------------------------
# pixels: the 64- and 128-pixel tile edges, M = 2048 (the 128 x 64 tile and the 3-way split start there), the counts at which
# m_tiles * n_tiles reaches 1024 (no K split) for 1, 2 and 3 cout tiles, the network's levels at batch 8, refused values
PIXELS = [1, 63, 64, 65, 200, 800, 2047, 2048, 2049, 3200, 12800, 21824, 21825, 32704, 32768, 65472, 65473, 204800, 0, -64]
PLAN_CIN = [64, 128, 256, 320, 384, 96]
PLAN_COUT = [64, 128, 192, 256, 100]

# (N, Hin, Win): M = 2047 / 2048 / 2049 at stride 1, the levels of the network, odd sizes, refused values
CONV2D_SHAPES = [(1, 23, 89), (1, 32, 64), (1, 3, 683), (8, 5, 5), (8, 10, 10), (8, 20, 20), (8, 40, 40), (8, 160, 160), (2, 41, 39),
                 (0, 8, 8)]
CONV2D_CIN = [64, 128, 384, 96]
CONV2D_COUT = [64, 256, 100]
KSIZE_STRIDE = [(1, 1), (1, 2), (3, 1), (3, 2), (2, 1), (5, 1), (3, 3)]

# the projection appends Cin2 / 64 steps to K: 36 + 1, + 2, + 3, + 5 steps and 1 + 1 ... (most do not divide by the split)
PROJ_SHAPES = [(1, 23, 89), (1, 32, 64), (8, 10, 10), (8, 20, 20), (8, 40, 40), (8, 160, 160)]
PROJ_CIN = [64, 256]
PROJ_COUT = [64, 256]
PROJ_KSIZE_STRIDE = [(1, 1), (1, 2), (3, 1), (3, 2)]
PROJ_CIN2 = [64, 128, 192, 320, 96, 0]

# ---- the tiled kernels ------------------------------------------------------------------------------------------------------
# (N, H, W): all four kinds (16 x 16, 40 x 4, 20 x 4, none), 199 / 200 work items at the 20- and 40-wide forms (with Cout 128 and
# 640), heights that are no multiple of 4, the 2^30-element limit from both sides, refused values
TILED_SHAPES = [(8, 160, 160), (8, 80, 80), (8, 40, 40), (8, 20, 20), (8, 10, 10), (1, 16, 16), (1, 48, 32), (199, 4, 20), (200, 4, 20),
                (199, 4, 40), (200, 4, 40), (50, 16, 40), (1, 4, 40), (3, 8, 40), (1, 6, 40), (1, 4, 20), (1, 18, 20), (2, 24, 24),
                (64, 256, 256), (63, 256, 256), (0, 16, 16), (1, 15, 17)]
TILED_CIN = [64, 128, 192, 256, 320, 384, 96]       # 2, 4, 6, 8, 10, 12 chunks of 32: divisible or not by 4 and by 6; a violation
TILED_COUT = [128, 256, 640, 64, 192]

# stride 2, (N, Hin, Win) of the INPUT: 16k x 8k outputs, the 40-wide form with an even and an odd output height, odd inputs, the
# limits (Cin: 2^30 input elements, Cout: 2^32)
S2_SHAPES = [(8, 320, 320), (8, 160, 160), (8, 80, 80), (8, 40, 40), (1, 16, 32), (1, 12, 80), (1, 10, 80), (1, 16, 80), (1, 17, 32),
             (1, 16, 33), (1, 32, 64), (4, 1024, 1024), (0, 16, 32)]
S2_CIN = [64, 128, 256, 96, 32]
S2_COUT = [128, 256, 896, 1024, 64, 192]


def grids():
    """The argument tuples of every pinned entry point, by section name."""
    return {
        'conv3x3': list(itertools.product(PIXELS, PLAN_CIN, PLAN_COUT)),
        'conv3x3_nhw': [(n, h, w, ci, co) for (n, h, w), ci, co in itertools.product(CONV2D_SHAPES, CONV2D_CIN, CONV2D_COUT)],
        'conv2d': [(n, h, w, ci, co, k, s)
                   for (n, h, w), ci, co, (k, s) in itertools.product(CONV2D_SHAPES, CONV2D_CIN, CONV2D_COUT, KSIZE_STRIDE)],
        'conv2d_proj': [(n, h, w, ci, co, k, s, c2) for (n, h, w), ci, co, (k, s), c2 in
                        itertools.product(PROJ_SHAPES, PROJ_CIN, PROJ_COUT, PROJ_KSIZE_STRIDE, PROJ_CIN2)],
        'tiled': [(n, h, w, ci, co) for (n, h, w), ci, co in itertools.product(TILED_SHAPES, TILED_CIN, TILED_COUT)],
        's2_tiled': [(n, h, w, ci, co) for (n, h, w), ci, co in itertools.product(S2_SHAPES, S2_CIN, S2_COUT)],
    }


def record(lib):
    """Rows of [arguments..., result(s)]: 'tiled' rows end in [supported, workspace_bytes], every other row in one value."""
    g = grids()
    return {
        'conv3x3': [[*a, lib.og_conv3x3_workspace_bytes(*a)] for a in g['conv3x3']],
        'conv3x3_nhw': [[*a, lib.og_conv3x3_workspace_bytes_nhw(*a)] for a in g['conv3x3_nhw']],
        'conv2d': [[*a, lib.og_conv2d_workspace_bytes(*a)] for a in g['conv2d']],
        'conv2d_proj': [[*a, lib.og_conv2d_proj_workspace_bytes(*a)] for a in g['conv2d_proj']],
        'tiled': [[*a, lib.og_conv3x3_tiled_supported(*a), lib.og_conv3x3_tiled_workspace_bytes(*a)] for a in g['tiled']],
        's2_tiled': [[*a, lib.og_conv3x3s2_tiled_supported(*a)] for a in g['s2_tiled']],
    }


def main():
    from offsetguided_amd import _lib
    rows = record(_lib.load())
    with open(GOLDEN, 'w') as f:
        f.write('{\n')
        for i, (name, rs) in enumerate(rows.items()):
            f.write(' "%s": [\n' % name)
            f.write(',\n'.join('  ' + json.dumps(r, separators=(',', ':')) for r in rs))
            f.write('\n ]%s\n' % (',' if i + 1 < len(rows) else ''))
        f.write('}\n')
    print(GOLDEN, {k: len(v) for k, v in rows.items()}, 'rows', sum(len(v) for v in rows.values()))


if __name__ == '__main__':
    main()
