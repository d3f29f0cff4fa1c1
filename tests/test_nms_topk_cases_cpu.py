"""The directed K1 planes of tests/nms_topk_cases.py, on the host: the two references (C oracle, numpy restatement) agree on every
case, and every case HAS the property it was built for -- recomputed here from the reference output and the host restatement of
K1's plan, not taken from the builder.  No GPU."""
import numpy as np
import pytest

import oracle
import nms_topk_cases as nc

NAMES = [c.name for c in nc.CASES]


def test_table_size():
    assert len(nc.CASES) == nc.N_CASES == len(set(NAMES))
    ks = {c.k for c in nc.CASES}
    assert ks == set(nc.K_VALUES)
    for k in ks:                                                  # every k meets the tie and the slot arithmetic
        assert {4, 7} <= {c.pattern for c in nc.CASES if c.k == k}
    for k in (32, 5):                                             # the full list, on VEC = 4 and on VEC = 1
        for g in ('g644x256', 'g324x125'):
            assert {c.pattern for c in nc.CASES if c.k == k and c.geom == g} == set(range(1, 11))
    assert {c.geom for c in nc.CASES} == set(nc.GEOMS)


def test_host_plan_of_the_geometries():
    p = {n: nc.plan(g.H, g.W, 32, g.aligned, g.entry == 'fused') for n, g in nc.GEOMS.items()}
    assert (p['g324x64'].nbands, p['g324x64'].nwaves, p['g324x64'].vec) == (5, 1, 4)
    assert (p['g644x256'].nbands, p['g644x256'].nwaves, p['g644x256'].vec, p['g644x256'].panel_cols) == (9, 2, 4, 128)
    assert (p['g324x125'].nwaves, p['g324x125'].vec, p['g324x125'].panel_cols) == (3, 1, 42)
    assert p['g5120x8'].nbands == 64 and p['g5120x8'].helper
    assert (p['g84x961'].nwaves, p['g84x961'].vec, p['g84x961'].helper) == (16, 1, False)
    assert (p['g644x256m'].vec, p['g644x256m'].nwaves, p['g644x256m'].nbands) == (1, 5, 9)
    assert (p['f161x64'].nwaves, p['f161x64'].panel_cols, p['f161x64'].nbands) == (2, 128, 9)
    assert p['f1280x8'].nbands == 64 and p['f81x16'].nbands == 5
    assert [(nc.plan(644, 256, k).t_band, nc.plan(644, 256, k).need, nc.plan(644, 256, k).cap) for k in (1, 2, 3, 5, 33, 100)] == \
        [(1, 1, 128), (1, 2, 128), (1, 3, 128), (2, 3, 128), (9, 4, 192), (25, 4, 320)]
    # the bins: 3 mantissa bits from 2^-30 up, clamped at both ends
    # (bin 0 = [2^-30, 1.125 * 2^-30) and everything below it)
    assert nc.bits_f32(nc.hist_edge_bits(1)) == np.float32(1.125 * 2.0 ** -30) and nc.bits_f32(nc.hist_edge_bits(255)) == np.float32(3.75)
    assert nc.hist_bin(1) == 0 and nc.hist_bin(nc.f32_bits(2.0 ** -30) - 1) == 0 and nc.hist_bin(nc.f32_bits(2.0 ** -30)) == 0
    assert nc.hist_bin(nc.f32_bits(3.75) - 1) == 254 and nc.hist_bin(nc.f32_bits(np.finfo(np.float32).max)) == 255
    for b in (1, 100, 224, 255):
        assert nc.hist_bin(nc.hist_edge_bits(b)) == b and nc.hist_bin(nc.hist_edge_bits(b) - 1) == b - 1


def _counts(pos, pl):
    """positive peaks per (band, wave panel) of one plane"""
    return np.array([[int(pos[pl.starts[b]:pl.starts[b + 1], c:c + pl.panel_cols].sum()) for c in range(0, pl.W, pl.panel_cols)]
                     for b in range(pl.nbands)])


@pytest.mark.parametrize("name", NAMES)
def test_case(name):
    case = nc.BY_NAME[name]
    g = nc.grid(case)
    pl, k, geom = g.plan, case.k, g.geom
    fused = geom.entry == 'fused'
    x = nc.build(name)
    assert x.shape[0] == 1 and x.shape[2:] == (geom.H // g.unit, geom.W // g.unit)
    assert 2 * (geom.H + geom.W) - 4 >= k and geom.H * geom.W >= k          # no case is refused or skipped anywhere
    hr = nc.hires(case, x)
    rs, ri, ry, rx = nc.reference(name)
    s2, i2 = nc.restate_nms_topk(hr, k)
    assert np.array_equal(rs, s2) and np.array_equal(np.signbit(rs), np.signbit(s2)) and np.array_equal(ri, i2)
    assert np.array_equal(ry, i2 // geom.W) and np.array_equal(rx, i2 % geom.W)
    if case.pattern in nc.PLAIN_PATTERNS and not fused:
        ps, pi, _, _ = nc.reference_plain(name)
        s3, i3 = nc.restate_topk(x, k)
        assert np.array_equal(ps, s3) and np.array_equal(pi, i3)

    nms = oracle.hmp_nms(hr)[0]
    pos = nms > 0
    band = np.searchsorted(np.asarray(pl.starts[1:]), ry[0], side='right')      # (C, k): band of every winner
    wave = rx[0] // pl.panel_cols
    kth = rs[0, :, k - 1]
    t, need = pl.t_band, pl.need

    if not fused and case.pattern not in (8,):                    # isolated peaks: no two within one pixel of each other
        for p in range(pos.shape[0]):
            q = np.pad(pos[p], 1).astype(np.int32)
            nb = sum(q[dy:dy + geom.H, dx:dx + geom.W] for dy in range(3) for dx in range(3))
            assert (nb[pos[p]] == 1).all()
            assert np.array_equal(nms[p], hr[0, p])               # and the planted values ARE the peaks

    if case.pattern == 1:
        assert (band == pl.nbands - 1).all() and (rs > 0).all()
        assert all(_counts(pos[0], pl)[b].sum() > 0 for b in range(pl.nbands))
    elif case.pattern == 2:
        assert (band == 0).all() and (rs > 0).all()
        assert all(_counts(pos[0], pl)[b].sum() > 0 for b in range(pl.nbands))
    elif case.pattern == 3:
        assert (rs == rs[0, 0, 0]).all() and (band == 0).all() and (wave == 0).all()
        cnt = _counts(nms[0] == rs[0, 0, 0], pl)
        assert (cnt > 0).all() and cnt.sum() >= 3 * k            # the same value waits in every band and panel
    elif case.pattern == 4:
        for p in range(2):
            ties = nms[p] == kth[p]
            assert kth[p] > 0 and ties.sum() >= 3 * k
            cnt = _counts(ties, pl)
            assert (cnt[1:] >= 2).all() and ((cnt[0] >= 2).all() if p == 0 else (cnt[0] == 0).all())
            n_above = int((nms[p] > kth[p]).sum())
            assert n_above == (k - 1) // g.mult * g.mult < k      # k - 1 distinct high peaks (fused: whole impulses)
            won = rs[0, p] == kth[p]
            assert won.sum() == k - n_above
            first_tie_band = band[p][won][0]
            assert (first_tie_band == 0) if p == 0 else (first_tie_band >= 1)
    elif case.pattern == 5:
        for e, b in enumerate(nc.EDGE_BINS):
            E = nc.hist_edge_bits(b)
            seen = set()
            for j, want in enumerate((E, E - 1, E + 1)):
                p = 3 * e + j
                assert nc.f32_bits(kth[p]) == want
                below = nc.bits_f32(want - 1)
                assert (nms[p] == below).sum() >= 2 * k and (nms[p] > kth[p]).sum() == k - 1
                seen.add((nc.hist_bin(want), nc.hist_bin(want - 1), nc.hist_bin(want + 1)))
            assert seen == {(b, b - 1, b), (b - 1, b - 1, b), (b, b, b)}       # each side of the edge, one ulp either way
    elif case.pattern == 6:
        bins = [np.array([nc.hist_bin(v) for v in nms[p][pos[p]].view(np.int32)]) for p in range(3)]
        assert (bins[0] == 0).all() and nms[0][pos[0]].view(np.int32).min() == 1 and nc.hist_bin(nc.f32_bits(kth[0])) == 0
        assert (nms[0][pos[0]] < np.float32(2.0 ** -30)).all() and len(bins[0]) == 3 * k
        assert (bins[1] == 255).all() and nms[1].max() == np.finfo(np.float32).max and nms[1][pos[1]].min() == np.float32(3.75)
        assert set(bins[2]) == {0, 255} and 0 < (bins[2] == 255).sum() < k and nc.hist_bin(nc.f32_bits(kth[2])) == 0
        assert np.isfinite(hr).all()
    elif case.pattern == 7:
        seen = set()
        for p, P in enumerate((need - 1, need)):
            main = nms[p] >= np.float32(0.1) if fused else pos[p]      # (fused: the blobs' small diagonal side lobes are peaks too)
            cnt = _counts(main, pl).sum(1)
            seen |= set(cnt.tolist())
            assert (cnt[:P] >= t).all() and (cnt[P:] < t).all()       # exactly P bands reach t_band
            if not fused:
                assert set(cnt[:P].tolist()) <= {t, t + 1}
            if P >= 1:
                lo_band = P - 1
                top_pub = nms[p][:pl.starts[P]].max()
                for b in range(P, pl.nbands):                        # the other bands: larger than any publishing peak, or filler below
                    v = nms[p][pl.starts[b]:pl.starts[b + 1]]
                    v = v[v >= np.float32(0.1)] if fused else v[v > np.float32(0.05)]
                    assert (v > top_pub).all()
                assert (band[p] == lo_band).any(), "the winners must reach into the lowest publishing band"
        if not fused and t >= 2:
            assert {t - 1, t} <= seen
        if not fused and k >= 31:
            assert {t - 1, t, t + 1} <= seen
    elif case.pattern == 8:
        H, W = geom.H, geom.W
        for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            assert pos[0, cy, cx]
        assert pos[0, 0].sum() > 4 and pos[0, H - 1].sum() > 4
        for s in range(pl.panel_cols, W, pl.panel_cols):             # both pixels of a plateau are peaks, one each side of the seam
            assert (pos[0, :, s - 1] & pos[0, :, s] & (nms[0, :, s - 1] == nms[0, :, s])).sum() >= 2, s
        for bs in pl.starts[1:-1]:
            assert (pos[0, bs - 1] & pos[0, bs] & (nms[0, bs - 1] == nms[0, bs])).sum() >= 2, bs
    elif case.pattern == 9:
        for p in range(2):
            n = int(pos[p].sum())
            assert n < k and (rs[0, p, n:] == 0).all() and (rs[0, p, :n] > 0).all()
            assert not pos[p][:pl.starts[-2]].any()
        assert fused or pos[0].sum() == k - 1
    elif case.pattern == 10:
        cnt = _counts(pos[0], pl)
        # four segments' worth per wave; the stride-4 grid cannot plant that many bumps in a 128-column panel: two there
        # (and a last panel that is narrower than the others -- 46 of 61 columns at W = 961 -- holds three)
        full = cnt[:, :-1] if pl.W % pl.panel_cols else cnt
        assert (full > (2 if fused else 4) * pl.cap).all() and (cnt > (2 if fused else 3) * pl.cap).all(), cnt.min()
        if not fused:
            v = nms[0][pos[0]]
            assert (np.diff(v) > 0).all()

    d = nc.decoy(case.geom, k, x.shape[1])
    assert d.shape == x.shape
    dn = oracle.hmp_nms(nc.hires(case, d))[0, 0]
    dcnt = _counts(dn >= np.float32(2.0), pl).sum(1)
    assert (dcnt >= t).all()
    if not fused:
        assert set(np.unique(dn)) == {np.float32(0), nc.DECOY_VALUE}
