"""Ground-truth encoder, CPU side of the sweep fixture (tests/golden/encoder_sweep.npz, taken from the imported reference by
tools/gen_golden_encoder_sweep.py): the C oracle is held to the reference on every case, so the GPU tests may use it as the
reference for inputs the fixture does not store (reversed persons, the seeded fuzz)."""
import numpy as np
import pytest

from encoder_sweep_common import (EDGE_GRIDS, FUZZ_SEEDS, HEADS, SWEEP_CASES, case_params, fuzz_config, load_sweep,
                                  oracle_outputs, skeleton_of)
from test_encoder import heatmaps_match


@pytest.mark.parametrize("case", SWEEP_CASES)
def test_oracle_matches_reference_sweep(case):
    g = load_sweep()
    j, prm = g[f"{case}_joints"], case_params(g, case)
    hm, jit, off, sc, ps = oracle_outputs(j, prm)
    assert heatmaps_match(hm, g[f"{case}_hm"], prm["clip"])
    assert np.array_equal(off, g[f"{case}_off"]) and np.array_equal(ps, g[f"{case}_pscale"])
    assert np.array_equal(sc, g[f"{case}_scale"], equal_nan=True)
    assert np.array_equal(jit, g[f"{case}_jitter"])


def test_sweep_fixture_covers_what_it_is_for():
    """The cases between them reach what tests/golden/encoder.npz leaves out."""
    g = load_sweep()
    assert list(g["cases"]) == SWEEP_CASES
    prm = {c: case_params(g, c) for c in SWEEP_CASES}
    persons = {c: g[f"{c}_joints"].shape[0] for c in SWEEP_CASES}
    col = lambda k: {p[k] for p in prm.values()}  # noqa: E731
    cells = {c: (p["in_w"] // p["stride"]) * (p["in_h"] // p["stride"]) for c, p in prm.items()}
    assert any(p["in_w"] != p["in_h"] and cells[c] % 256 and cells[c] > 256 for c, p in prm.items())
    assert col("head") == set(HEADS) and {2, 4, 8} <= col("stride")
    assert len(col("sigma") - {7}) >= 2 and len(col("clip") - {0.01}) >= 1
    for k, default in (("fill_jitter", 3), ("fill_scale", 7)):
        other = col(k) - {default}
        assert any(v % 2 for v in other) and any(v % 2 == 0 for v in other), (k, other)
    for c, p in prm.items():
        if p["min_jscale"] > 1:
            j = g[f"{c}_joints"]
            s = j[:, :, 3][j[:, :, 2] > 0]
            assert (s < p["min_jscale"]).any() and (s == p["min_jscale"]).any() and (s > p["min_jscale"]).any(), c
    assert any(p["min_jscale"] > 1 for p in prm.values())
    assert any(n > 1020 for n in persons.values()) and any(513 <= n <= 1020 for n in persons.values())
    # the planted case: unlabelled fillers in front of a tied pair at the staging boundary of the offsets kernel, and the
    # ties are real -- reversing the persons changes offsets, keypoint scales and jitter
    j, p = g["planted_joints"], prm["planted"]
    assert not (j[:511, :, 2] > 0).any() and (j[511, :, 2] > 0).any() and (j[512, :, 2] > 0).any()
    fwd, rev = oracle_outputs(j, p), oracle_outputs(j[::-1], p)
    assert not np.array_equal(fwd[1], rev[1]) and not np.array_equal(fwd[2], rev[2])
    assert not np.array_equal(fwd[3], rev[3], equal_nan=True)
    assert np.array_equal(fwd[0], rev[0])      # the heat maps are a maximum: order-free


def test_fuzz_configurations_span_the_parameter_space():
    """The seeded configurations of the GPU fuzz test (drawn without a GPU): 1, 255, 256 and 257 cells, every stride, every
    skeleton, both staging boundaries, empty images next to crowded ones, input sizes off the stride's multiples."""
    cfgs = [fuzz_config(s) for s in FUZZ_SEEDS]
    assert len(cfgs) >= 24
    cells = {(p["in_w"] // p["stride"]) * (p["in_h"] // p["stride"]) for p, _ in cfgs}
    assert {1, 255, 256, 257} <= cells and len(EDGE_GRIDS) <= len(cfgs)
    assert {p["stride"] for p, _ in cfgs} == {2, 4, 8} and {p["head"] for p, _ in cfgs} == set(HEADS)
    assert {p["min_jscale"] for p, _ in cfgs} == {1.0, 2.5, 4.0} and len({p["sigma"] for p, _ in cfgs}) >= 5
    assert len({p["clip"] for p, _ in cfgs}) >= 3
    for k in ("fill_jitter", "fill_scale"):
        assert any(p[k] % 2 for p, _ in cfgs) and any(p[k] % 2 == 0 for p, _ in cfgs)
    assert any(p["in_w"] % p["stride"] for p, _ in cfgs)
    counts = [[j.shape[0] for j in js] for _, js in cfgs]
    assert any(max(c) > 1020 for c in counts) and any(512 < max(c) <= 1020 for c in counts)
    assert any(0 in c and max(c) > 0 for c in counts) and all(len(c) >= 2 for c in counts)
    prm, js = cfgs[3]
    again = fuzz_config(FUZZ_SEEDS[3])
    assert again[0] == prm and all(np.array_equal(a, b) for a, b in zip(again[1], js))
    assert all(len(skeleton_of(h)) > 0 for h in HEADS)
