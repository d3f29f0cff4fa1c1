"""Directed planes for K1 (csrc/nms_topk.hip: 3x3 max-NMS + per-plane top-k) -- shared by tests/test_nms_topk_cases_cpu.py and
tests/test_gpu_nms_topk_warm.py.  No GPU code; importing it needs no device.

References.  The primary one is the C oracle (oracle.nms_topk / oracle.topk, oracle.bicubic4 in front of the fused entry).  Beside
it stands `restate_nms_topk` / `restate_topk`, plain numpy that shares no code with the oracle or the kernels: 3x3 maximum with zero
padding, keep v where v == max else 0, the k best of the flattened plane ordered by (-value, index) through a stable sort.

HOST RESTATEMENT OF THE PLAN (`plan`, `hist_bin`, `hist_edge_bits`).  It repeats make_plan / run_topk of nms_topk.hip ONLY TO PLACE
INPUTS -- where the 80-row bands, the wave panels and the histogram bins of a geometry lie -- and is no reference for any result.

A case is one (1, C, H, W) float32 tensor (for the fused entry: the stride-4 tensor, (1, C, H/4, W/4)) plus a note: the pattern it
was built from and the numbers the CPU test recomputes from the reference output.  Peaks are isolated pixels on a lattice (no two
within one pixel of each other) unless the pattern says otherwise; for the fused entry a "peak" is an impulse on the stride-4 grid,
five pixels from the next one and off the border, so that every impulse becomes the same x4 bicubic blob (a 2 x 2 plateau: four
peaks of one value per impulse).

Patterns (the number is the `pattern` field of a case):
   1 ascending by row      every later band holds larger peaks: all k winners sit in the last band
   2 descending by row     all k winners sit in the first band, every later band is cut by the published bound
   3 all equal             one value everywhere; the winners are the k lowest indices: band 0, wave 0
   4 tie at the k-th place k - 1 distinct high peaks, >= 3k peaks of the k-th value.  Plane 0: at least two of them in every band and
                           panel.  Plane 1: the same without band 0, so that the one tie that wins does NOT lie in the first band
                           (both readings of "in every band" and "the lowest-index one not in the first band" are built)
   5 bin edges             nine planes = three edges E = hist_edge_bits(b) x (k-th best == E, nextafter(E, 0), nextafter(E, inf));
                           2k peaks one ulp below the k-th best, (k - 1) // 2 peaks one ulp above it
   6 clamped bins          plane 0: all peaks in (0, 2^-30) incl. the smallest denormal; plane 1: all in [3.75, FLT_MAX]; plane 2: both
                           ranges, fewer than k in the upper one (the k-th best lies in bin 0 with bin 255 populated)
   7 slot arithmetic       plane 0: exactly need - 1 bands reach t_band peaks, plane 1: exactly need.  Those bands (the first ones) hold
                           t_band or t_band + 1 peaks in descending value ranges; every other band ends in peaks larger than anything in
                           them, fewer than t_band each, and so few in all that the k winners reach into the LOWEST publishing band: a
                           bound taken one rank too high loses them.  One other band holds exactly t_band - 1 peaks
   8 seams                 two-pixel plateaus across every panel seam and every band boundary, isolated peaks in the corners and along
                           the first and last row
   9 few peaks             fewer than k positive peaks, all in the last band (plane 0: k - 1, plane 1: k // 2): the zero-fill path
  10 segment overflow      a lattice of step 2 with strictly increasing values in scan order: every compaction raises tau to a value
                           the next row exceeds
"""
import functools
import os
from collections import namedtuple

import numpy as np

for _knob in ("OG_NMS_ROWS", "OG_K1_WAVE_LISTS", "OG_K1_HIST_MBITS"):
    assert _knob not in os.environ, f"{_knob} is set: the host restatement of K1's plan below holds for the defaults only"

# ---------------------------------------------------------------------------------- host restatement of the plan (input placement)
BAND_ROWS, INTERIOR, FUSED_INTERIOR, MAX_WAVES = 80, 62, 58, 16
HIST_MBITS, HIST_BINS = 3, 256
HIST_SHIFT = 23 - HIST_MBITS
HIST_BASE = (127 + 2 - (HIST_BINS >> HIST_MBITS)) << HIST_MBITS        # bin 0 starts at 2^-30, bin 255 at 3.75

Plan = namedtuple('Plan', 'H W k vec fused nbands starts nwaves panel_cols t_band need cap helper')


def _ceil(a, b):
    return -(-a // b)


def plan(H, W, k, aligned=True, fused=False):
    """Where K1 cuts an (H, W) plane (H, W: the hi-res size also for the fused entry).  starts: nbands + 1 row numbers; panel_cols:
    columns per wave panel (the seams are its multiples)."""
    vec = 4 if (W % 4 == 0 and aligned) else 1
    strips = _ceil(W, vec)
    nwaves = _ceil(strips, INTERIOR)
    panel_strips = _ceil(strips, nwaves)
    if fused:
        vec, w4 = 4, W // 4
        nwaves = _ceil(w4, FUSED_INTERIOR)
        panel_strips = _ceil(w4, nwaves)
    rows = min(max(BAND_ROWS, _ceil(H, 64)), H)
    nb = _ceil(H, rows)
    starts = [((b * H) // nb) & ~3 for b in range(nb)] + [H]
    t_band = (k + 3) // 4
    return Plan(H, W, k, vec, fused, nb, starts, nwaves, panel_strips * vec, t_band, _ceil(k, t_band), _ceil(2 * k + 64, 64) * 64,
                nb <= 64 and nwaves < MAX_WAVES)


def f32_bits(v):
    return int(np.asarray(v, np.float32).view(np.int32))


def bits_f32(b):
    return np.asarray(b, np.int32).view(np.float32)[()]


def hist_bin(bits):
    return min(max((int(bits) >> HIST_SHIFT) - HIST_BASE, 0), HIST_BINS - 1)


def hist_edge_bits(b):
    return 1 if b == 0 else (b + HIST_BASE) << HIST_SHIFT


# ---------------------------------------------------------------------------------- the second reference (plain numpy)
def _nms_map(x):
    x = np.asarray(x, np.float32)
    H, W = x.shape[-2:]
    p = np.zeros(x.shape[:-2] + (H + 2, W + 2), np.float32)
    p[..., 1:-1, 1:-1] = x
    m = p[..., 0:H, 0:W]
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, p[..., dy:dy + H, dx:dx + W])
    return np.where(x == m, x, np.float32(0))


def restate_topk(x, k):
    """(scores, flat indices) of the k best per plane, ordered by (-value, index)."""
    x = np.asarray(x, np.float32)
    flat = x.reshape(x.shape[0], x.shape[1], -1)
    order = np.argsort(-flat, axis=-1, kind='stable')[..., :k]
    return np.take_along_axis(flat, order, -1), order.astype(np.int64)


def restate_nms_topk(x, k):
    return restate_topk(_nms_map(x), k)


# ---------------------------------------------------------------------------------- geometries
Geom = namedtuple('Geom', 'name H W entry aligned')        # H, W: hi-res; entry 'nms' (joint_dets) or 'fused' (joint_dets_lowres)
GEOMS = {g.name: g for g in [
    Geom('g324x64', 324, 64, 'nms', True),        # 5 bands, one wave
    Geom('g644x256', 644, 256, 'nms', True),      # 9 bands, two waves, VEC = 4, seam at column 128
    Geom('g324x125', 324, 125, 'nms', True),      # VEC = 1, three waves, seams at 42 and 84
    Geom('g5120x8', 5120, 8, 'nms', True),        # 64 bands: the limit of the slot scan
    Geom('g84x961', 84, 961, 'nms', True),        # VEC = 1, 16 waves: the histogram pointer is live, no helper wave
    Geom('g644x256m', 644, 256, 'nms', False),    # storage offset of one float: VEC = 1 by misalignment at W % 4 == 0
    Geom('f81x16', 324, 64, 'fused', True),
    Geom('f161x64', 644, 256, 'fused', True),
    Geom('f1280x8', 5120, 32, 'fused', True),     # 64 bands through the fused entry
]}


class Grid:
    """The grid a case is planted on (hi-res pixels, or stride-4 pixels for the fused entry) with K1's bands and panels in its units."""

    def __init__(self, geom, k):
        self.geom, self.k = geom, k
        self.plan = p = plan(geom.H, geom.W, k, geom.aligned, geom.entry == 'fused')
        self.unit = u = 4 if p.fused else 1                     # hi-res pixels per grid pixel
        self.mult = 4 if p.fused else 1                         # peaks per planted site
        self.h, self.w = geom.H // u, geom.W // u
        self.band_rows = [s // u for s in p.starts]
        self.seams = [c // u for c in range(p.panel_cols, geom.W, p.panel_cols)]
        self.nb, self.npanels = p.nbands, len(self.seams) + 1
        if p.fused:                                             # equal blobs: five apart, off the border
            self.step, self.off_y, self.off_x = 5, 2, (2 if self.w > 4 else 0)
        else:
            self.step, self.off_y, self.off_x = 8, 0, 0
        self.step_x = self.step if self.w >= 16 else (2 if not p.fused else 5)

    def band_of(self, ys):
        return np.searchsorted(np.asarray(self.band_rows[1:]), ys, side='right')

    def panel_of(self, xs):
        return np.searchsorted(np.asarray(self.seams), xs, side='right') if self.seams else np.zeros(len(xs), np.int64)

    def lattice(self, dy=None, dx=None):
        """-> ys, xs of the lattice sites in scan order (the fused grid leaves its last row and column free)"""
        dy, dx = dy or self.step, dx or self.step_x
        ys = np.arange(self.off_y, self.h - (1 if self.plan.fused else 0), dy)
        xs = np.arange(self.off_x, self.w - (1 if self.plan.fused and self.w > 4 else 0), dx)
        yy, xx = np.meshgrid(ys, xs, indexing='ij')
        return yy.ravel(), xx.ravel()

    def spread(self, n, taken=None):
        """n lattice sites spread over the plane (a fixed stride permutation of the scan order), none of them in `taken`"""
        ys, xs = self.lattice()
        m = len(ys)
        stride = next(s for s in (389, 251, 127, 61, 31, 13, 7, 5, 3, 1) if np.gcd(s, m) == 1 and s < max(m, 2))
        order = (np.arange(m) * stride) % m
        if taken is not None:
            order = np.array([i for i in order if (ys[i], xs[i]) not in taken], np.int64)
        assert len(order) >= n, (self.geom.name, n, len(order))
        return ys[order[:n]], xs[order[:n]]

    def zeros(self, c):
        return np.zeros((c, self.h, self.w), np.float32)


def _ladder(n, lo, hi):
    v = np.linspace(lo, hi, n, dtype=np.float64).astype(np.float32) if n > 1 else np.full(n, hi, np.float32)
    assert len(np.unique(v)) == n
    return v


# ---------------------------------------------------------------------------------- patterns
def _p_ramp(g, descending):
    ys, xs = g.lattice()
    v = _ladder(len(ys), 0.05, 0.95)
    x = g.zeros(1)
    x[0, ys, xs] = v[::-1] if descending else v
    return x


def p1(g):
    return _p_ramp(g, False)


def p2(g):
    return _p_ramp(g, True)


def p3(g):
    ys, xs = g.lattice()
    pan = g.panel_of(xs)
    n0 = max(1, int(np.sum((ys == ys[0]) & (pan == 0))))
    first = ys[0] + g.step * _ceil(g.k, n0 * g.mult)                # the other panels start below panel 0's k first peaks
    keep = (pan == 0) | (ys >= first)
    x = g.zeros(1)
    x[0, ys[keep], xs[keep]] = 0.5
    return x


TIE = np.float32(0.25)


def p4(g):
    k = g.k
    ys, xs = g.lattice()
    band, pan = g.band_of(ys), g.panel_of(xs)
    x = g.zeros(2)
    for plane in range(2):
        bands = [b for b in range(g.nb) if not (plane == 1 and b == 0)]
        per_cell = max(2, _ceil(_ceil(3 * k, g.mult), len(bands) * g.npanels))
        taken = set()
        for b in bands:
            for p in range(g.npanels):
                idx = np.flatnonzero((band == b) & (pan == p))
                assert len(idx) >= per_cell + 1, (g.geom.name, k, b, p, len(idx), per_cell)
                idx = idx[:per_cell]
                x[plane, ys[idx], xs[idx]] = TIE
                taken.update(zip(ys[idx].tolist(), xs[idx].tolist()))
        nhigh = (k - 1) // g.mult
        hy, hx = g.spread(nhigh, taken)
        x[plane, hy, hx] = _ladder(nhigh, 1.0, 2.0)
    return x


EDGE_BINS = (1, 224, 255)          # 1.125 * 2^-30 (the first real edge), 0.25, 3.75 (the last one)


def p5(g):
    k = g.k
    x = g.zeros(9)
    for e, b in enumerate(EDGE_BINS):
        E = bits_f32(hist_edge_bits(b))
        for j, kth in enumerate((E, np.nextafter(E, np.float32(0)), np.nextafter(E, np.float32(np.inf)))):
            n_up = (k - 1) // 2
            ys, xs = g.spread(k - 1 + 1 + 2 * k)
            vals = np.concatenate([np.full(n_up, np.nextafter(kth, np.float32(np.inf)), np.float32),
                                   (_ladder(k - 1 - n_up, 2.0, 3.9) * kth).astype(np.float32),
                                   [kth], np.full(2 * k, np.nextafter(kth, np.float32(0)), np.float32)])
            x[3 * e + j, ys, xs] = vals
    return x


LOW_TOP_BITS, HIGH_LO_BITS, HIGH_TOP_BITS = 0x307fffff, 0x40700000, 0x7f7fffff      # < 2^-30; 3.75; FLT_MAX


def p6(g):
    k = g.k
    n = 3 * k
    low = (1 + np.arange(n, dtype=np.int64) * ((LOW_TOP_BITS - 1) // max(n - 1, 1))).astype(np.int32)
    if n >= 4:
        low[1], low[2] = 2, 0x007fffff                                                # more denormals: the second smallest, the largest
    high = (HIGH_LO_BITS + np.arange(n, dtype=np.int64) * ((HIGH_TOP_BITS - HIGH_LO_BITS) // max(n - 1, 1))).astype(np.int32)
    high[-1] = HIGH_TOP_BITS
    n_hi = k // 2
    mixed = np.concatenate([high[:n_hi], low[:n - n_hi]])
    x = g.zeros(3)
    ys, xs = g.spread(n)
    for plane, bits in enumerate((low, high, mixed)):
        assert len(np.unique(bits)) == n
        x[plane, ys, xs] = bits.view(np.float32)
    return x


def p7(g):
    k, pl, mult = g.k, g.plan, g.mult
    t, need = pl.t_band, pl.need
    ys, xs = g.lattice()
    band = g.band_of(ys)
    pub_sites = _ceil(t, mult)                                   # sites that make a band reach t_band peaks
    x = g.zeros(2)
    for plane, P in enumerate((need - 1, need)):
        assert g.nb >= P + 1, (g.geom.name, k)
        # peaks that may lie above the lowest publishing band while it still holds a winner
        budget = k - 1 - max(P - 1, 0) * pub_sites * mult
        extra = 1 if (P >= 2 and budget >= 2 * mult) else 0
        budget -= extra * mult
        for j in range(P):                                       # publishing bands: the first P, descending value ranges
            idx = np.flatnonzero(band == j)
            cnt = pub_sites + (extra if j == 0 else 0)
            assert len(idx) >= cnt
            x[plane, ys[idx[:cnt]], xs[idx[:cnt]]] = _ladder(cnt, 0.55 - 0.1 * j, 0.6 - 0.1 * j)
        large_ok = mult < t                                      # a site's peaks must stay below t_band in their band
        for r, b in enumerate(range(P, g.nb)):                   # the other bands: one large site at their END, while the budget lasts
            idx = np.flatnonzero(band == b)
            n_large = 1 if (large_ok and budget >= mult) else 0
            if n_large:
                budget -= mult
                x[plane, ys[idx[-1]], xs[idx[-1]]] = np.float32(1.0 + 0.01 * r)
            if r == 0 and mult == 1 and t >= 2:                  # exactly t_band - 1 peaks in this band: small ones fill it up
                n_small = t - 1 - n_large
                x[plane, ys[idx[:n_small]], xs[idx[:n_small]]] = _ladder(n_small, 0.01, 0.02)
    return x


def p8(g):
    x = g.zeros(1)
    occ = np.zeros((g.h + 2, g.w + 2), bool)
    vals = iter(_ladder(20000, 0.1, 0.9))
    step = 8 if not g.plan.fused else 3

    def plant(pix):
        if any(not (0 <= y < g.h and 0 <= xx < g.w) for y, xx in pix):
            return
        if any(occ[y:y + 3, xx:xx + 3].any() for y, xx in pix):
            return
        v = next(vals)
        for y, xx in pix:
            x[0, y, xx] = v
        for y, xx in pix:
            occ[y + 1, xx + 1] = True

    for cy, cx in ((0, 0), (0, g.w - 1), (g.h - 1, 0), (g.h - 1, g.w - 1)):
        plant([(cy, cx)])
    for bs in g.band_rows[1:-1]:                                 # vertical plateaus across every band boundary
        for cx in range(3, g.w, step):
            plant([(bs - 1, cx), (bs, cx)])
    for s in g.seams:                                            # horizontal plateaus across every panel seam
        for cy in range(4, g.h, step):
            plant([(cy, s - 1), (cy, s)])
    for cx in range(2, g.w, max(step // 2, 2)):                  # first and last row
        plant([(0, cx)])
        plant([(g.h - 1, cx)])
    return x


def p9(g):
    k = g.k
    ys, xs = g.lattice()
    last = np.flatnonzero(g.band_of(ys) == g.nb - 1)
    x = g.zeros(2)
    per_site = 8 if g.plan.fused else 1                          # (a blob's four diagonal side lobes are positive peaks too)
    for plane, n in enumerate(((k - 1) // per_site, (k // 2) // per_site)):
        assert len(last) >= n
        idx = last[len(last) - n:]
        x[plane, ys[idx], xs[idx]] = _ladder(n, 0.1, 0.9)
    return x


def p10(g):
    x = g.zeros(1)
    if g.plan.fused:                                             # stride-4 checkerboard: the blobs overlap, one bump per impulse
        yy, xx = np.meshgrid(np.arange(g.h), np.arange(g.w), indexing='ij')
        sel = ((yy + xx) % 2 == 0).ravel()
        ys, xs = yy.ravel()[sel], xx.ravel()[sel]
    else:
        ys, xs = g.lattice(2, 2)
    x[0, ys, xs] = _ladder(len(ys), 0.01, 1.0)
    return x


PATTERNS = {1: p1, 2: p2, 3: p3, 4: p4, 5: p5, 6: p6, 7: p7, 8: p8, 9: p9, 10: p10}
PLAIN_PATTERNS = (3, 4, 6, 10)            # the ones that also mean something to plain top-k (og_topk_channel_f32)
DECOY_VALUE = np.float32(3.5)

Case = namedtuple('Case', 'name geom k pattern')


def _cases():
    out = []

    def add(gname, k, patterns):
        for p in patterns:
            out.append(Case(f'{gname}_k{k}_p{p}', gname, k, p))

    for k in (32, 5):                                            # the full list
        add('g644x256', k, range(1, 11))
        add('g324x125', k, range(1, 11))
    add('f161x64', 32, (1, 2, 3, 4, 7, 8, 9, 10))
    add('f161x64', 5, (1, 2, 3, 4, 8, 9, 10))                    # (pattern 7 needs t_band > 4 there: four peaks per impulse)
    add('g324x64', 32, (1, 2, 4, 7, 8))
    add('g5120x8', 32, (1, 2, 4, 7, 9))
    add('g84x961', 32, (1, 2, 4, 8, 10))                         # (two bands: no room for pattern 7)
    add('g644x256m', 32, (2, 4, 5, 7, 8, 10))
    add('f81x16', 32, (2, 4, 7))
    add('f1280x8', 5, (2, 4))                                    # (16 peaks per band there)
    for k in (1, 2, 3, 31, 33, 63, 64, 65, 100):                 # every other k: the tie and the slot arithmetic
        add('g644x256', k, (4, 7))
    for k in (3, 33, 100):
        add('g324x125', k, (4, 7))
    for k in (31, 64):                                           # (k = 33: three impulses a band overshoot t_band by three)
        add('f161x64', k, (4, 7))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
N_CASES = 109
K_VALUES = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 100)


def grid(case):
    return Grid(GEOMS[case.geom], case.k)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> the case's input, (1, C, h, w) float32 (read-only: shared between tests)"""
    case = BY_NAME[name]
    x = PATTERNS[case.pattern](grid(case))[None]
    assert x.dtype == np.float32 and np.isfinite(x).all()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def decoy(gname, k, c):
    """Peaks of 3.5 on the whole lattice (at least t_band in every band), C planes of the same geometry"""
    g = Grid(GEOMS[gname], k)
    ys, xs = g.lattice()
    x = g.zeros(c)
    x[:, ys, xs] = DECOY_VALUE
    x = x[None]
    x.setflags(write=False)
    return x


def hires(case, x):
    """The plane K1 ranks: the input, or its x4 bicubic upsample for the fused entry"""
    import oracle
    return oracle.bicubic4(x) if GEOMS[case.geom].entry == 'fused' else np.asarray(x)


@functools.lru_cache(maxsize=None)
def reference(name):
    """oracle.nms_topk of the case -> (scores, inds, ys, xs), computed once (read-only)"""
    import oracle
    case = BY_NAME[name]
    out = oracle.nms_topk(hires(case, build(name)), case.k)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_plain(name):
    """oracle.topk of the case's tensor as it stands (no NMS): the reference of plain top-k"""
    import oracle
    case = BY_NAME[name]
    out = oracle.topk(build(name), case.k)
    for a in out:
        a.setflags(write=False)
    return out
