"""The six fused loss kernels of csrc/losses.hip restated in numpy float64, and the seeded inputs the fp64 loss tests share
(tests/test_losses_fp64_cpu.py holds this file to models/losses.py in torch float64; tests/test_gpu_losses_fp64.py holds the
kernels to it).  No torch in the arithmetic.

Every function takes the float32 arrays exactly as the kernel receives them -- pred / gt / ps (N, C, hw), logb (N, C/2, hw),
mask bytes (N, hw), scalar parameters already rounded to float32 -- widens them to float64 and returns a `Ref`:

  sum          float64 sum of the kept terms                        abs_sum   sum of |term| (for the summation bound)
  count        integer number of kept terms                         kept      bool, the element (vector kernels: the pair) counts
  grad         float64 d sum / d pred, 0 on dropped elements        borderline  bool, see below
  gbound       float64 bound on |float32 gradient - grad|           ill       bool, laplace: gbound is set by conditioning (below)
  chk, chk_bound   what a float32 kernel is held to: grad and gbound, except on `cont` elements (offset l1 with sqrt, below)
  scale64      magnitude of the terms a float64 evaluation of grad rounds (the CPU comparison with torch float64 uses it)
  grad_logb / gbound_logb / ill_logb / scale64_logb                 laplace only

Definitions (models/losses.py and the comment blocks of csrc/losses.hip): an element is a candidate where its mask byte is
non-zero and its target is finite (vector kernels: r = |(dx, dy)| finite; offset kernel: gt / ps finite).  focal and l2 keep
every candidate; the others keep v >= margin with v = |p - g|, |p / ps - g / ps|, r, or logb + r exp(-logb) (a NaN or negative
laplace value fails the comparison).  The kept term is v, or sqrt(v) with sqrt_re.  Gradients are those of the SUM; norm'(0)
= 0, and |x|^gamma has derivative 0 at x = 0 (for gamma < 1 the torch formulation has NaN = inf * 0 there, like the norm
backward next to an undefined target; the kernels write the exact 0 in both places).

u = 2^-24 is the unit roundoff of float32: one correctly rounded operation has relative error <= u.  As libog_decoder.so is
compiled (no fast-math, the compiler's default correctly rounded float32 divide and sqrt) division and sqrtf are correctly
rounded, but HIP's math-API accuracy table gives sqrtf, expf and powf 1 ulp = 2 u each, and that is what is charged.  The
bounds are first order in u; SLACK = 1.01 covers the higher orders.

Borderline windows.  An element is borderline where the keep-or-drop decision (or the sign of an l1 gradient) of a correctly
rounded float32 evaluation may differ from exact arithmetic:
  masked l1   d = fl(p - g) is one rounding: |d32 - d| <= u |d|.  Window |e - margin| <= u e.
  offset l1   d = fl(fl(p/ps) - fl(g/ps)): |d32 - d| <= E = u (|p/ps| + |g/ps|) + u |d| (each quotient and the difference charged
              only where not exactly representable).  Window |e - margin| <= E, and e <= E for a kept element (sign of d).
  vector l1   dx, dy one rounding each (u), squares 3 u, their sum 4 u, the root halves that and adds its own 2 u: r32 within
              4 u r.  Window |r - margin| <= 4 u r.  isfinite(r): dx^2 + dy^2 overflows float32 although r would be finite; the
              restatement drops the pair like the kernel, window (1 +- 8 u) FLT_MAX on the sum of squares.
  laplace     exp 2 u, r exp(-logb) 7 u, the sum adds u |v|: Ev = 7 u r exp(-logb) + u |v|.  Window |v - margin| <= Ev.
  focal       t >= tau compares two float32 numbers: exact, the window is empty.  1 - s is 0 only for s == 1: the sign of
              1 - st is exact too.
  offset l1   gt / ps at the float32 overflow edge: window (1 +- 4 u) FLT_MAX.
A value that is exactly representable at every step (p - g == margin with both float32, p == g, ps a power of two ...) is
evaluated without error by any float32 implementation: it is not borderline and follows the `>=` and sign rules.

Gradient bounds (gbound), roundings on the path from the inputs to g:
  l2          g = fl(p - g): 1 u |g|.
  masked l1   plain: g = +-1, exact (bound 0).  sqrt: g = +-0.5 / sqrt(e): e u (halved), sqrtf 2 u, divide u: 4 u |g|.
  offset l1   plain: g = +-1 / ps, one divide: u |g|.  sqrt: (0.5 E / e + 4 u) |g| -- sgn / ps u, sqrtf 2 u, divide u, and the error
              of e = |p/ps - g/ps| passes through the root with factor 1/2.  E / e is the condition number of the subtraction.
              Where it outweighs the roundings (0.5 E / e > 4 u, that is |p/ps| + |g/ps| > 7 e or so) the element is `cont`: chk
              is the float64 continuation from d32 = fl(fl(p/ps) - fl(g/ps)), which IEEE arithmetic fixes bit for bit (the only
              float32 arithmetic in this file), and chk_bound = 4 u |chk| covers every later operation: sgn / ps, sqrtf, divide.
  focal       g = A + B, A = d f, B = 0.5 d^2 f'.  gamma = 1: 3 u (|A| + |B|) + u |g| <= 4 u (|A| + |B|).  Otherwise powf(a, y)
              costs |y| u (the rounding of a = |1 - s|) + 2 u: A (gamma + 4) u, B (|gamma - 1| + 7) u, the sum one more:
              (max(gamma + 4, |gamma - 1| + 7) + 1) u (|A| + |B|).  The bound is relative to |A| + |B|, not to |g|: the two terms
              cancel at s = s* / 3.
  vector l1   g = dx * (k / r): r 4 u, divide u, dx u, product u = 7 u; sqrt: k = 0.5 / sqrt(r) adds 2 u + 2 u + u = 12 u.  Charged
              (rel_k + 7 u) |g| with rel_k = 0 or 0.5 Ev / v + 3 u; laplace (rel_k + 10 u) |g|: exp 2 u and k * inv u more.
  laplace     grad_logb = k (1 - r exp(-logb)): |k| ((rel_k + 2 u) |1 - r inv| + 7 u r inv); `ill` where 0.5 Ev / v > 4 u.
              `ill_logb` also where r inv lies within a factor 2 of 1: the subtraction 1 - r inv is then exact and hands the 7 u
              of r inv on as an absolute error of up to 4.2e-7, whatever is left of the difference.  The device's expf is not
              correctly rounded, so fl(r inv) cannot be restated bit for bit and there is no continuation as for offset l1: on
              `ill` / `ill_logb` elements whose derived bound exceeds rtol 1e-5 / atol 1e-7 the derived bound stands alone.
"""
import collections

import numpy as np

from offsetguided_amd import synth

U = 2.0 ** -24
SLACK = 1.01
F32_MAX = float(np.finfo(np.float32).max)
MARGIN = np.float32(1e-5)           # models/losses.py MARGIN / MARGIN2 / TAU as the kernels receive them
MARGIN2 = np.float32(0.1)
TAU = np.float32(0.01)

Ref = collections.namedtuple('Ref', 'sum count grad kept borderline abs_sum gbound ill grad_logb gbound_logb ill_logb chk chk_bound cont scale64 scale64_logb')

KERNELS = ('focal', 'offset', 'l2', 'ml1', 'vector', 'laplace')
ENTRY = {'focal': 'og_focal_l2_loss_f32', 'offset': 'og_offset_l1_loss_f32', 'l2': 'og_l2_loss_f32', 'ml1': 'og_masked_l1_loss_f32',
         'vector': 'og_vector_l1_loss_f32', 'laplace': 'og_laplace_loss_f32'}
HAS_V = ('l2', 'ml1', 'vector', 'laplace')         # kernels with the 16-byte path


def _f64(*xs):
    return [np.asarray(x).astype(np.float64) for x in xs]


def _repr32(x):
    """True where the float64 value is a float32 number (a float32 operation with that exact result does not round)."""
    with np.errstate(over='ignore', invalid='ignore'):
        return x.astype(np.float32).astype(np.float64) == x


def _lab(mask, shape):
    n, c, hw = shape
    return np.broadcast_to(np.asarray(mask).reshape(n, 1, hw) != 0, shape)


def _finish(term, kept, grad, gbound, borderline, ill=None, grad_logb=None, gbound_logb=None, ill_logb=None, chk=None,
            chk_bound=None, cont=None, scale64=None, scale64_logb=None):
    term = np.where(kept, term, 0.0)
    zero = np.zeros_like(kept)
    return Ref(float(term.sum()), int(kept.sum()), grad, kept, borderline, float(np.abs(term).sum()), gbound,
               zero if ill is None else ill & kept, grad_logb, gbound_logb, ill_logb, grad if chk is None else chk,
               gbound if chk_bound is None else chk_bound, zero if cont is None else cont,
               np.abs(grad) if scale64 is None else scale64, scale64_logb)


def focal_l2(pred, gt, mask, tau, gamma):
    s, t = _f64(pred, gt)
    tau, gamma = float(np.float32(tau)), float(np.float32(gamma))
    kept = _lab(mask, s.shape) & np.isfinite(t)
    t = np.where(kept, t, 0.0)
    fg = t >= tau
    om = np.where(fg, 1.0 - s, s)
    a, d = np.abs(om), s - t
    da = np.sign(om) * np.where(fg, -1.0, 1.0)
    if gamma == 1.0:
        f, df, k = a, da, 4.0
    else:
        f = a ** gamma
        with np.errstate(divide='ignore'):
            df = np.where(a > 0, gamma * a ** (gamma - 1.0), 0.0) * da
        k = max(gamma + 4.0, abs(gamma - 1.0) + 7.0) + 1.0
    A, B = d * f, 0.5 * d * d * df
    grad = np.where(kept, A + B, 0.0)
    gbound = np.where(kept, SLACK * k * U * (np.abs(A) + np.abs(B)), 0.0)
    return _finish(0.5 * d * d * f, kept, grad, gbound, np.zeros_like(kept), scale64=np.where(kept, np.abs(A) + np.abs(B), 0.0))


def offset_l1(pred, gt, ps, mask, margin, sqrt_re):
    p, t, sc = _f64(pred, gt, ps)
    margin = float(np.float32(margin))
    with np.errstate(all='ignore'):
        tn = t / sc
        fin = np.isfinite(t) & np.isfinite(tn) & (np.abs(tn) <= F32_MAX)
        edge = np.isfinite(t) & np.isfinite(tn) & (np.abs(np.abs(tn) / F32_MAX - 1.0) <= 4 * U)
    cand = _lab(mask, p.shape) & fin
    tn = np.where(cand, tn, 0.0)
    pn = p / sc
    d = pn - tn
    e = np.abs(d)
    rp, rt = _repr32(pn), _repr32(tn)
    exact = rp & rt & _repr32(d)
    E = U * (np.abs(pn) * ~rp + np.abs(tn) * ~rt) + U * e * ~exact
    kept = cand & (e >= margin)
    borderline = cand & ((~exact & ((np.abs(e - margin) <= SLACK * E) | (kept & (e <= SLACK * E)))) | edge)
    es = np.where(kept, e, 1.0)
    sg = np.sign(d) / sc
    if sqrt_re:
        r = np.sqrt(es)
        term, grad, rel = r, sg * 0.5 / r, 0.5 * E / es + 4 * U
        grad = np.where(kept, grad, 0.0)
        gbound = SLACK * rel * np.abs(grad)
        # where the cancellation in p/ps - g/ps outweighs the roundings, the kernel is held to the float64 continuation from
        # the float32 difference itself (IEEE division and subtraction: numpy's float32 gives the same bits as any device)
        with np.errstate(all='ignore'):
            p32, t32, s32 = (np.asarray(x, np.float32) for x in (pred, gt, ps))
            d32 = (p32 / s32 - t32 / s32).astype(np.float64)
        e32 = np.abs(d32)
        cont = kept & (0.5 * E / es > 4 * U) & (e32 >= margin) & (np.sign(d32) == np.sign(d))
        e32 = np.where(cont, e32, 1.0)
        chk = np.where(cont, np.sign(d32) / sc * 0.5 / np.sqrt(e32), grad)
        chk_bound = np.where(cont, SLACK * 4 * U * np.abs(chk), gbound)
        scale64 = np.abs(grad) * (1.0 + 0.5 * (np.abs(pn) + np.abs(tn)) / es)
        return _finish(term, kept, grad, gbound, borderline, None, chk=chk, chk_bound=chk_bound, cont=cont, scale64=scale64)
    term, grad, rel = e, sg, np.where(_repr32(1.0 / sc), 0.0, U)
    grad = np.where(kept, grad, 0.0)
    return _finish(term, kept, grad, SLACK * rel * np.abs(grad), borderline)


def l2(pred, gt, mask):
    p, t = _f64(pred, gt)
    kept = _lab(mask, p.shape) & np.isfinite(t)
    d = p - np.where(kept, t, 0.0)
    grad = np.where(kept, d, 0.0)
    return _finish(0.5 * d * d, kept, grad, SLACK * U * np.abs(grad) * ~_repr32(d), np.zeros_like(kept))


def masked_l1(pred, gt, mask, margin, sqrt_re):
    p, t = _f64(pred, gt)
    margin = float(np.float32(margin))
    cand = _lab(mask, p.shape) & np.isfinite(t)
    d = p - np.where(cand, t, 0.0)
    e = np.abs(d)
    exact = _repr32(d)
    kept = cand & (e >= margin)
    borderline = cand & ~exact & (np.abs(e - margin) <= SLACK * U * e)
    if sqrt_re:
        r = np.sqrt(np.where(kept, e, 1.0))
        term, grad, rel = r, np.sign(d) * 0.5 / r, 4 * U
    else:
        term, grad, rel = e, np.sign(d), 0.0
    grad = np.where(kept, grad, 0.0)
    return _finish(term, kept, grad, SLACK * rel * np.abs(grad), borderline)


def _vector(pred, gt, logb, mask, margin, sqrt_re):
    p, t = _f64(pred, gt)
    margin = float(np.float32(margin))
    n, c, hw = p.shape
    L = c // 2
    p, t = p.reshape(n, L, 2, hw), t.reshape(n, L, 2, hw)
    with np.errstate(all='ignore'):
        dx, dy = p[:, :, 0] - t[:, :, 0], p[:, :, 1] - t[:, :, 1]
        s2 = dx * dx + dy * dy
        fin = np.isfinite(s2) & (s2 <= F32_MAX)
        edge = np.isfinite(s2) & (np.abs(s2 / F32_MAX - 1.0) <= 8 * U)
    cand = _lab(mask, (n, L, hw)) & fin
    dx, dy = np.where(cand, dx, 0.0), np.where(cand, dy, 0.0)
    r = np.sqrt(dx * dx + dy * dy)
    if logb is None:
        inv, ri, v = 1.0, r, r
        Ev = 4 * U * r
    else:
        lb, = _f64(logb)
        with np.errstate(all='ignore'):
            inv = np.exp(-lb)
            ri = r * inv
            v = lb + ri                                       # NaN for a NaN logb, and for -inf (-inf + inf, or 0 * inf at r = 0)
            Ev = np.where(r > 0, 7 * U * ri + U * np.abs(v), 0.0)
    with np.errstate(invalid='ignore'):
        kept = cand & (v >= margin)
        borderline = cand & (((Ev > 0) & (np.abs(v - margin) <= SLACK * Ev)) | edge)
    vs = np.where(kept, v, 1.0)
    inv, ri, Ev = [np.where(kept, x, 0.0) for x in np.broadcast_arrays(inv, ri, Ev, kept)[:3]]
    if sqrt_re:
        s = np.sqrt(vs)
        term, k, rel_k = s, 0.5 / s, 0.5 * Ev / vs + 3 * U
        ill = 0.5 * Ev / vs > 4 * U
    else:
        term, k, rel_k, ill = vs, np.ones_like(vs), np.zeros_like(vs), None
    kr = np.where(kept & (r > 0), k * inv / np.where(r > 0, r, 1.0), 0.0)
    grad = np.stack([dx * kr, dy * kr], axis=2).reshape(n, c, hw)
    gbound = SLACK * np.stack([rel_k + (7 if logb is None else 10) * U] * 2, axis=2).reshape(n, c, hw) * np.abs(grad)
    two = lambda x: np.stack([x] * 2, axis=2).reshape(n, c, hw)  # noqa: E731
    lbm = 0.0 if logb is None else np.where(kept, np.abs(np.where(kept, lb, 0.0)), 0.0)
    cancel = np.ones_like(vs) + (0.5 * (lbm + ri) / vs if sqrt_re else 0.0)            # float64 conditioning of v = logb + r inv under the root
    scale64, scale64_b = np.abs(grad) * two(cancel), None
    gl = gbl = ill_b = None
    if logb is not None:
        gl = np.where(kept, k * (1.0 - ri), 0.0)
        gbl = np.where(kept, SLACK * np.abs(k) * ((rel_k + 2 * U) * np.abs(1.0 - ri) + 7 * U * ri), 0.0)
        ill_b = kept & (np.abs(1.0 - ri) < 0.5 * ri)
        if ill is not None:
            ill_b |= ill & kept
        scale64_b = np.where(kept, np.abs(k) * (1.0 + ri) * cancel, 0.0)
    return _finish(term, kept, grad, gbound, borderline, ill, gl, gbl, ill_b, scale64=scale64, scale64_logb=scale64_b)


def vector_l1(pred, gt, mask, margin, sqrt_re):
    return _vector(pred, gt, None, mask, margin, sqrt_re)


def laplace(pred, gt, logb, mask, margin, sqrt_re):
    return _vector(pred, gt, logb, mask, margin, sqrt_re)


def reference(case):
    """Ref of a case from make_case()."""
    k, a = case['kernel'], case
    if k == 'focal':
        return focal_l2(a['pred'], a['gt'], a['mask'], a['tau'], a['gamma'])
    if k == 'offset':
        return offset_l1(a['pred'], a['gt'], a['ps'], a['mask'], a['margin'], a['sqrt_re'])
    if k == 'l2':
        return l2(a['pred'], a['gt'], a['mask'])
    if k == 'ml1':
        return masked_l1(a['pred'], a['gt'], a['mask'], a['margin'], a['sqrt_re'])
    if k == 'vector':
        return vector_l1(a['pred'], a['gt'], a['mask'], a['margin'], a['sqrt_re'])
    return laplace(a['pred'], a['gt'], a['logb'], a['mask'], a['margin'], a['sqrt_re'])


# ---- launch geometry of csrc/losses.hip (loss_grid: at most 2048 blocks of 256 lanes, a lane owns V elements per pass) ----
CAP = 2048 * 256


def geometry(kernel, n, cp, hw, aligned=True):
    """(V, units, blocks, m, W): m = the longest per-lane accumulation chain, W = atomics per accumulator (one per wave)."""
    v = 4 if kernel in HAS_V and hw % 4 == 0 and aligned else 1
    units = n * cp * hw // v
    blocks = min((units + 255) // 256, 2048)
    passes = -(-units // (blocks * 256))
    return v, units, blocks, passes * v, blocks * 4


# ---- shapes: (name, N, C', hw) with C' the channels (element-wise kernels) or the (x, y) pairs (vector kernels) ----
TRAIN = {'focal': ('train', 8, 17, 16384), 'l2': ('train', 8, 17, 16384), 'ml1': ('train', 8, 17, 16384),
         'offset': ('train', 8, 38, 16384), 'vector': ('train', 8, 19, 16384), 'laplace': ('train', 8, 19, 16384)}
# units CAP - 1, CAP, CAP + 1 on the 16-byte path (hw % 4 == 0) and on the 4-byte path (hw % 4 != 0); 2^19 - 1 is prime
CAP_SHAPES = [('v4_cap-1', 1, 1, 4 * (CAP - 1)), ('v4_cap', 2, 2, CAP), ('v4_cap+1', 1, 3, 4 * (CAP + 1) // 3),
              ('v1_cap-1', 1, 1, CAP - 1), ('v1_cap', 512, 512, 2), ('v1_cap+1', 1, 3, (CAP + 1) // 3)]
SMALL_V1 = [('v1_u1', 1, 1, 1), ('v1_u63', 1, 1, 63), ('v1_u64', 2, 16, 2), ('v1_u65', 1, 1, 65), ('v1_u255', 1, 1, 255),
            ('v1_u256', 2, 64, 2), ('v1_u257', 1, 1, 257)]
SMALL_V4 = [(f'v4_u{u}', 1, 1, 4 * u) for u in (1, 63, 64, 65, 255, 256, 257)]
HW_MOD = [(f'hw{hw}', 2, 3, hw) for hw in (40, 41, 42, 43)]
SPECIAL = [('masked_image', 3, 2, 44), ('no_finite_target', 2, 2, 36)]
LARGEST = ('train', 'v4_cap+1')                    # left out of the torch float64 comparison on the CPU
TINY = 300                                         # below this many elements a case need not have kept, dropped AND masked ones


def variants(kernel):
    if kernel == 'focal':
        return [dict(gamma=np.float32(g), tau=np.float32(t)) for g in (1, 2, 0.5) for t in (0.01, 0.5)]
    if kernel == 'l2':
        return [dict()]
    if kernel in ('offset', 'ml1'):
        return [dict(margin=m, sqrt_re=s) for m in (MARGIN, MARGIN2) for s in (0, 1)]
    return [dict(margin=MARGIN, sqrt_re=s) for s in (0, 1)]


def vtag(v):
    return '-'.join(f'{k[0]}{float(x):g}' for k, x in v.items()) or 'plain'


def case_list(kernel, big=True):
    """[(id, shape, variant, seed, flags)] of a kernel: every variant at the training shape, at `v4_cap` and `v1_cap+1` and at the
    small shapes; the other cap shapes take the variants in turn."""
    out = []
    vs = variants(kernel)
    shapes = ([TRAIN[kernel]] + CAP_SHAPES if big else []) + SMALL_V1 + SMALL_V4 + HW_MOD + SPECIAL
    for si, shape in enumerate(shapes):
        rotate = shape[0] in ('v4_cap-1', 'v4_cap+1', 'v1_cap-1', 'v1_cap')
        for vi, v in enumerate(vs):
            if rotate and vi != si % len(vs):
                continue
            flags = dict(masked_image=1 if shape[0] == 'masked_image' else None, no_targets=shape[0] == 'no_finite_target')
            out.append((f'{kernel}-{shape[0]}-{vtag(v)}', shape, v, 1000 * (KERNELS.index(kernel) + 1) + 10 * si + vi, flags))
    return out


EXACT = {'focal': dict(gamma=np.float32(1), tau=np.float32(0.5)), 'l2': dict(), 'ml1': dict(margin=MARGIN2, sqrt_re=0),
         'offset': dict(margin=MARGIN, sqrt_re=0)}
QUANTUM = {'focal': 2.0 ** -4, 'l2': 2.0 ** -5, 'ml1': 2.0 ** -2, 'offset': 2.0 ** -1}


def exact_case_list(kernel):
    """The dyadic input sets of a kernel without sqrtf / expf / powf on the summed term: training shape and two cap shapes."""
    shapes = [TRAIN[kernel], CAP_SHAPES[2], CAP_SHAPES[5]]
    return [(f'{kernel}-{s[0]}-exact', s, EXACT[kernel], 9000 + 10 * KERNELS.index(kernel) + i, dict(exact=True))
            for i, s in enumerate(shapes)]


MASK_BYTES = np.array([0, 1, 2, 255, 1, 2, 255, 1], np.uint8)


def make_case(kernel, shape, variant, seed, masked_image=None, no_targets=False, exact=False):
    """dict of float32 / uint8 numpy arrays and float32 parameters, as the entry point of `kernel` takes them."""
    name, n, cp, hw = shape
    c = cp * 2 if kernel in ('vector', 'laplace') else cp
    rng = synth.HashRng(seed)
    tot = n * c * hw
    uni = lambda lo, hi, ch=c: rng.uniform(n * ch * hw, lo, hi).astype(np.float32).reshape(n, ch, hw)  # noqa: E731
    cls = lambda hi, ch=c: rng.integers(n * ch * hw, 0, hi).reshape(n, ch, hw)  # noqa: E731
    case = dict(kernel=kernel, name=name, n=n, c=c, cp=cp, hw=hw, exact=exact, quantum=QUANTUM.get(kernel) if exact else None,
                **variant)
    mask = MASK_BYTES[rng.integers(n * hw, 0, 7)].reshape(n, hw)          # the four bytes of a dword differ
    if masked_image is not None:
        mask[masked_image] = 0
    case['mask'] = mask
    inf, nan = np.float32(np.inf), np.float32(np.nan)

    def holes(t, q, frac):
        """+inf in `frac` of the targets, a few -inf and NaN."""
        t[q < int(1000 * frac)] = inf
        t[q == 998] = -inf
        t[q == 999] = nan

    if exact:
        q = cls(999)
        if kernel == 'focal':               # s in {-1/2, 0, 1/2, 1}, t in {0, 1/2, 1}, tau 1/2: terms are multiples of 2^-4
            pred = np.array([0, 0, 1, 1, 1, 2, 2, -1], np.float32)[cls(7)] * np.float32(0.5)
            gt = np.array([0, 0, 0, 0, 0, 0, 1, 2], np.float32)[cls(7)] * np.float32(0.5)
            holes(gt, q, 0.02)
        elif kernel == 'offset':            # p, t in {0, 1, 2}, ps in {1, 2}: e is a multiple of 1/2
            pred, gt = cls(2).astype(np.float32), cls(2).astype(np.float32)
            case['ps'] = np.array(np.broadcast_to(np.array([1, 2], np.float32)[cls(1, 1)], (n, c, hw)))
            holes(gt, q, 0.3)
        else:                               # p, t in {0, 1/4, 1/2, 3/4}: 0.5 d^2 is a multiple of 2^-5, |d| of 2^-2
            pred, gt = cls(3).astype(np.float32) * np.float32(0.25), cls(3).astype(np.float32) * np.float32(0.25)
            holes(gt, q, 0.3)
        case['pred'], case['gt'] = pred, gt
        return case

    q = cls(999)
    if kernel == 'focal':
        gt = uni(0, 1) * (uni(0, 1) > np.float32(0.8))
        pred = uni(-0.2, 1.1)                                   # outside [0, 1]: 1 - st negative
        z = cls(31)
        pred[z == 0], pred[z == 1] = 0.0, 1.0                   # |1 - st| = 0 on either side
        gt[q == 997] = case['tau']                              # exactly on the threshold: foreground
        gt[(q == 996) & (z == 1)] = 1.0
        holes(gt, q, 0.01)
    elif kernel == 'l2':
        gt, pred = uni(0, 1), uni(-0.2, 1.1)
        holes(gt, q, 0.05)
    elif kernel == 'ml1':                                       # keypoint scales: NaN outside the patches
        gt, pred = uni(1, 12), uni(0, 13)
        near = cls(9) == 0
        pred[near] = gt[near] + np.float32(0.05)                # inside MARGIN2, outside MARGIN
        gt[q < 600] = nan
        gt[(q >= 600) & (q < 610)] = inf
        gt[q == 998] = -inf
    else:                                                       # offsets
        gt, pred = uni(-60, 60), uni(-60, 60)
        same = cls(9) == 0
        if kernel == 'offset':
            pred[same] = gt[same]
            case['ps'] = np.array(np.broadcast_to(uni(20, 300, 1), (n, c, hw)))
            holes(gt, q, 0.3)
        else:
            pair = lambda m: np.repeat(m, 2, axis=1)  # noqa: E731
            same, closeby, q2 = pair(cls(9, cp) == 0), pair(cls(19, cp) == 0), pair(cls(999, cp))
            pred[same] = gt[same]                               # r = 0: the laplace value is logb, negative in part
            pred[closeby & ~same] = (gt + np.float32(0.03125))[closeby & ~same]
            holes(gt, q2, 0.6)
            gt[q == 997] = inf                                  # one component only
            if kernel == 'laplace':
                lb, ql = uni(-2, 3, cp), cls(999, cp)
                lb[ql == 0], lb[ql == 1] = nan, -inf            # +inf would make the value, and the sum, +inf as in torch
                case['logb'] = lb
    if kernel in ('ml1', 'offset'):                             # |d| exactly on the margin, one float32 below it, twice it
        m = np.float32(case['margin'])
        for code, (pv, tv) in enumerate([(m, 0), (-m, 0), (np.nextafter(m, np.float32(0)), 0), (2 * m, m), (0, m)]):
            sel = q == 990 + code
            pred[sel], gt[sel] = pv, tv
            if kernel == 'offset':
                case['ps'][sel] = 1.0
    if no_targets:
        gt[:] = inf
        gt.reshape(-1)[::3] = nan
    case['pred'], case['gt'] = pred, gt
    assert pred.shape == gt.shape == (n, c, hw) and tot == pred.size
    return case


def check_conditions(case, ref):
    """The input conditions every generated case must meet (asserted on the CPU; the GPU tests rely on them)."""
    nb = int(ref.borderline.sum())
    assert nb <= 4, f'{nb} borderline elements'
    assert ref.count < 2 ** 24
    lab = _lab(case['mask'], ref.kept.shape)
    if case['exact']:
        quanta = ref.abs_sum / case['quantum']
        assert quanta < 2 ** 24 and quanta == int(quanta), quanta
        assert nb == 0
    special = case['name'] in ('no_finite_target',)
    if ref.kept.size >= TINY and not special:
        assert ref.kept.any() and (~ref.kept & lab).any() and (~lab).any(), 'needs kept, dropped and masked elements'
    if case['name'] == 'no_finite_target':
        assert ref.count == 0 and ref.sum == 0.0
    if case['name'] == 'masked_image':
        assert not ref.kept[1].any() and ref.kept[0].any()
