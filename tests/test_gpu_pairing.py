"""The limb pairing (og_collect::limb_rows, csrc/collect_body.h) on the directed cases of tests/pairing_cases.py, every route that
accepts a case against the reference's stored output (tests/golden/pairing_edges.npz): og_collect_limbs_f32 on the stored lists
(int64 indices), og_generate_limbs_f32 on the planted heat maps (the in-launch pairing: int indices), offsets gathered from hi-res
maps / sampled from the stride-4 maps / flip-merged on load / refined on the spot (scored_off), the scale head in modes 1..3, the
jitter head in modes 1 and 3, 4-component offsets.  Both kernels run whole-wave groups: the half-wave GROUP = 32 variant the body's
comment speaks of is not instantiated in the library and is not tested here.  EXACT_LIMB_COLS bit for bit, the score within
SCORE_TOL, the returned lists equal to the stored ones.

The cases past the stored ones (pairing_cases.DIGEST: the K on both sides of the collect fallback of og_generate_limbs_f32, the scale
head on 4-component offsets, scale and jitter heads together, the 44-limb skeleton at K = 33 / 65 / 100) are compared with the C
oracle's rows, which pairing_cases.load holds to the SHA-256 of the reference's.

The forms that start from stride-4 heat maps (fused, fused-flip, with heads, with scored_off) cannot have peaks planted exactly -- a
single stride-4 cell upsamples to a 2 x 2 plateau of equal pixels, a top-k tie: they run on bump scenes (pairing_cases.build_fused)
against the oracle's lists and pairing, rows with both ends above the threshold; the directed offset / scale / jitter maps of the
cases over the bump heat maps (ScoredArgs in the launch, FlipHeadsArgs on exact and perturbed mirrors) on EVERY row."""
import numpy as np
import pytest
import torch

import oracle
import pairing_cases as pc
from helpers import assert_limbs_match
from offsetguided_amd import _lib
from offsetguided_amd.config import coco_data as cd
from offsetguided_amd.decoder.offset import scored_offset

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4      # the project's limb-score tolerance (tests/test_gpu_parity.py)
NAMES = [c.name for c in pc.CASES]
PLAIN = [c.name for c in pc.STORED if c.heads == 'none' and c.nd == 2 and c.skeleton == 'omp19']
FALLBACK = [c.name for c in pc.CASES if c.name.startswith('fallback')]
PLAIN44 = [c.name for c in pc.CASES if c.skeleton == 'omp44']


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def run(sk, n, hw, k, dev, nd=2, lists=None, own=False, ws=None, **form):
    """One call with the descriptor fields `form` (numpy arrays go to the device): og_collect_limbs_f32 on `lists` = (scores, inds),
    or og_generate_limbs_f32 -> limbs (N,L,k,13), returned scores, inds (None for the collect call), all numpy.  `own`: no list
    outputs are given -- the lists are read back from the workspace, [tickets | top-k | inds | scores].  `ws`: the workspace to use
    (a second, warm launch)."""
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    form = {f: torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v for f, v in form.items()}
    limbs = torch.full((n, len(sk), k, 13), float('nan'), device=dev)
    d = _lib.LimbsDesc(N=n, C=17, H=hw[0], W=hw[1], jf=_lib.int_table([a for a, _ in sk], dev), jt=_lib.int_table([b for _, b in sk], dev),
                       L=len(sk), k=k, thre_hmp=pc.THRE, min_len=pc.MIN_LEN, resize_factor=1.0, limbs=limbs, vector_nd=nd, **form)
    if lists is not None:
        sc, ix = (torch.tensor(a).to(dev) for a in lists)
        _lib.check(lib.og_collect_limbs_f32(_lib.ptr(sc), _lib.ptr(ix), d, st), lib)
        return limbs.cpu().numpy(), None, None
    sc = torch.full((n, 17, k), float('nan'), device=dev)
    ix = torch.full((n, 17, k), -1, dtype=torch.int64, device=dev)
    if not own:
        d.topk_scores, d.topk_inds = sc.data_ptr(), ix.data_ptr()
    if ws is None:
        ws = torch.zeros(lib.og_generate_limbs_workspace_bytes(n, 17, hw[0], hw[1], k), dtype=torch.uint8, device=dev)
    _lib.check(lib.og_generate_limbs_f32(d, _lib.ptr(ws), ws.numel(), st), lib)
    if own:
        at = 65536 + (lib.og_topk_workspace_bytes(n * 17, hw[0], hw[1], k) + 255) // 256 * 256
        ix = ws[at:at + n * 17 * k * 8].view(torch.int64).view(n, 17, k)
        sc = ws[at + n * 17 * k * 8:at + n * 17 * k * 12].view(torch.float32).view(n, 17, k)
    out = limbs.cpu().numpy(), sc.cpu().numpy(), ix.cpu().numpy()
    assert int(ws[:61440].view(torch.int32).abs().sum()) == 0, "the reserved head of the workspace must stay zero"
    return out


def head_routes(case, scene, exp):
    """[(tag, descriptor fields of the head, expected limbs)]: every mode the case's head has"""
    if case.heads == 'both':     # every scale mode with every jitter mode
        plain, j = pc.Case(case.name, case.K, case.H, case.W, case.skeleton, case.nd, 'scale'), scene['jit_lr']
        return [(f'{tag}+{jt}', dict(head, **jh), ref) for tag, head, ref in head_routes(plain, scene, exp)
                for jt, jh in (('jitter1', dict(jitter=oracle.bilinear4(j), jitter_mode=1)), ('jitter3', dict(jitter=j, jitter_mode=3)))]
    if case.heads == 'scale':
        s = scene['scl_lr']
        return [('scale1/bicubic', dict(scales=oracle.bicubic4(s), scales_mode=1), exp['limbs_bicubic']),
                ('scale1/bilinear', dict(scales=oracle.bilinear4(s), scales_mode=1), exp['limbs_bilinear']),
                ('scale2', dict(scales=s, scales_mode=2), exp['limbs_bicubic']), ('scale3', dict(scales=s, scales_mode=3), exp['limbs_bilinear'])]
    if case.heads == 'jitter':
        j = scene['jit_lr']
        return [('jitter1', dict(jitter=oracle.bilinear4(j), jitter_mode=1), exp['limbs']), ('jitter3', dict(jitter=j, jitter_mode=3), exp['limbs'])]
    return [('', {}, exp['limbs'])]


def offset_routes(scene):
    return [('hires', dict(offs=oracle.bilinear4(scene['off_lr']), off_lowres=0)), ('stride4', dict(offs=scene['off_lr'], off_lowres=1))]


def check_coverage(case, scene, exp):
    if case.name not in _COUNTS:     # once per case: the counts are those of the reference's values, whatever route is under test
        jit_hr = oracle.bilinear4(scene['jit_lr']) if scene['jit_lr'] is not None else None
        scl_hr = oracle.bicubic4(scene['scl_lr']) if scene['scl_lr'] is not None else None
        _COUNTS[case.name] = pc.counts(case, exp['scores'], exp['inds'], exp['limbs' if 'limbs' in exp else 'limbs_bicubic'],
                                       oracle.bilinear4(scene['off_lr']), jit_hr, scl_hr)
    cnt = _COUNTS[case.name]
    assert cnt and all(v >= 1 for v in cnt.values()), cnt


_COUNTS = {}


@pytest.mark.parametrize("name", NAMES)
def test_collect_on_the_stored_lists(dev, name):
    case, scene, exp = pc.load(name)
    sk = pc.skeleton(case)
    for h_tag, head, ref in head_routes(case, scene, exp):
        for o_tag, offs in offset_routes(scene):
            got, _, _ = run(sk, pc.N_IMAGES, (case.H, case.W), case.K, dev, case.nd, lists=(exp['scores'], exp['inds']), **offs, **head)
            assert not np.isnan(got).any(), (h_tag, o_tag)
            assert_limbs_match(ref, got, SCORE_TOL)
    check_coverage(case, scene, exp)


@pytest.mark.parametrize("name", NAMES)
def test_generate_on_the_planted_maps(dev, name):
    """The in-launch pairing of og_generate_limbs_f32: the lists it selects are the planted ones, its limbs the reference's."""
    case, scene, exp = pc.load(name)
    sk = pc.skeleton(case)
    for h_tag, head, ref in head_routes(case, scene, exp):
        for o_tag, offs in offset_routes(scene):
            got, sc, ix = run(sk, pc.N_IMAGES, (case.H, case.W), case.K, dev, case.nd, hmps=scene['hm_hr'], **offs, **head)
            assert (sc == exp['scores']).all() and (ix == exp['inds']).all(), (h_tag, o_tag)
            assert_limbs_match(ref, got, SCORE_TOL)
    check_coverage(case, scene, exp)


def weights(case):
    """stride-4 heat maps for scored_off to weigh with: dyadic, non-negative, a fifth of the cells zero"""
    w = pc._dyadic(77 + case.K, (pc.N_IMAGES, 17, case.H // 4, case.W // 4), -16, 63, 64)
    return np.maximum(w, 0).astype(np.float32)


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("name", PLAIN + FALLBACK)
def test_scored_offsets_refined_inside_the_pairing(dev, name, ks):
    """ScoredArgs on the stored lists (og_collect_limbs_f32 reads hmps as the weights): the pairing on offsets refined in front by the
    CPU formulation of scored_offset, which is bit-identical to the reference's."""
    case, scene, exp = pc.load(name)
    sk, w = pc.skeleton(case), weights(case)
    jf, jt = [a for a, _ in sk], [b for _, b in sk]
    refined = scored_offset(torch.from_numpy(w), torch.from_numpy(scene['off_lr']), jf, jt, kernel_size=ks).numpy()
    ref = oracle.collect_limbs(exp['scores'], exp['inds'], refined, True, (case.H, case.W), sk, pc.THRE, pc.MIN_LEN)
    got, _, _ = run(sk, pc.N_IMAGES, (case.H, case.W), case.K, dev, lists=(exp['scores'], exp['inds']), hmps=w, hm_lowres=1,
                    offs=scene['off_lr'], off_lowres=1, score_ksize=ks)
    assert_limbs_match(ref, got, SCORE_TOL)
    if ks == 3:
        assert (ref[..., 8] != exp['limbs'][..., 8]).any(), "the refinement is meant to move guide points"


def flip_tables(sk):
    perm, reserve = cd.offset_hflip(cd.COCO_KEYPOINTS, sk)
    return cd.heatmap_hflip(cd.COCO_KEYPOINTS), perm, reserve, [1 if l in reserve else 0 for l in range(len(sk))]


def mirrored(off_lr, perm):
    """The offsets the mirrored image of the case would give: limb perm[l] of the mirror holds limb l flipped along W, x negated --
    flip_augment (decoder/factory.py:129-138) folds them back onto the case's own offsets, exactly (dyadic values)."""
    n, c, h, w = off_lr.shape
    a = off_lr.reshape(n, c // 2, 2, h, w)
    b = np.empty_like(a)
    b[:, list(perm)] = a[..., ::-1]
    b[:, :, 0] *= np.float32(-1)
    return np.ascontiguousarray(b.reshape(n, c, h, w))


@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("name", PLAIN + PLAIN44 + [f'fallback_k{pc.IN_LAUNCH_K}'])      # (past it the fold is refused: below)
def test_flip_folded_offsets_over_the_planted_maps(dev, name, perturbed):
    """limb_perm + reserve_mask without kp_perm: the offsets of [images | mirrored images] merged on load, the planted heat maps as they
    are.  The exact mirror of the case merges back to the case's offsets: the limbs are the REFERENCE's stored ones.  With a dyadic
    perturbation on the mirrored half (so that the second half matters) the expected value is the pairing on oracle.flip_merge's offsets."""
    case, scene, exp = pc.load(name)
    sk, n = pc.skeleton(case), pc.N_IMAGES
    kp, perm, reserve, keep = flip_tables(sk)
    assert sorted(perm) == list(range(len(sk)))
    mirror = mirrored(scene['off_lr'], perm)
    if perturbed:
        mirror = mirror + pc._dyadic(55 + case.K, mirror.shape, -48, 47, 4)
    pair = np.concatenate([scene['off_lr'], mirror])
    _, merged = oracle.flip_merge(np.zeros((2 * n, 17) + pair.shape[2:], np.float32), pair, kp, perm, reserve)
    if perturbed:
        ref = oracle.collect_limbs(exp['scores'], exp['inds'], merged, True, (case.H, case.W), sk, pc.THRE, pc.MIN_LEN)
        assert (ref[..., 8] != exp["limbs"][..., 8]).any(), "the perturbation is meant to move guide points"
    else:
        assert (merged == scene['off_lr']).all()
        ref = exp['limbs']
    got, sc, ix = run(sk, n, (case.H, case.W), case.K, dev, hmps=scene['hm_hr'], offs=pair, off_lowres=1,
                      limb_perm=_lib.int_table(perm, dev), reserve_mask=_lib.int_table(keep, dev))
    assert (sc == exp['scores']).all() and (ix == exp['inds']).all()
    assert_limbs_match(ref, got, SCORE_TOL)


# ---------------------------------------------------------------------------------- the forms that start from stride-4 heat maps
FUSED_FORMS = ['fused', 'fused_scored1', 'fused_scored3', 'fused_heads', 'fused_flip', 'fused_flip_scored3', 'fused_flip_heads',
               'fused_flip_heads_bilinear', 'fused_flip_heads_scored3']


@pytest.mark.parametrize("form", FUSED_FORMS)
@pytest.mark.parametrize("K", pc.FUSED_K)
def test_fused_forms_against_the_oracle(dev, K, form):
    sk, n, hw = pc.SKELETONS['omp19'], pc.N_IMAGES, (64, 64)
    jf, jt = [a for a, _ in sk], [b for _, b in sk]
    hm, off, scl, jit = pc.build_fused(K)
    flip, heads, ks = 'flip' in form, 'heads' in form, int(form[-1]) if 'scored' in form else 0
    mode = 3 if 'bilinear' in form else 2
    kp, perm, reserve, keep = flip_tables(sk)
    fields = dict(hm_lowres=1, off_lowres=1, score_ksize=ks)
    if flip:
        fields.update(hmps=hm, offs=off, kp_perm=_lib.int_table(kp, dev), limb_perm=_lib.int_table(perm, dev),
                      reserve_mask=_lib.int_table(keep, dev))
        mh, mo = oracle.flip_merge(hm, off, kp, perm, reserve)
        mj = jit[n:][..., ::-1].copy()
        mj[:, 0::2] *= np.float32(-1)
        ms, mj = (scl[:n] + scl[n:, list(kp)][..., ::-1]) / np.float32(2), (jit[:n] + mj) / np.float32(2)
        h_scl, h_jit = scl, jit
    else:
        mh, mo, ms, mj = (np.ascontiguousarray(a[:n]) for a in (hm, off, scl, jit))
        fields.update(hmps=mh, offs=mo)
        h_scl, h_jit = ms, mj
    if heads:
        fields.update(scales=h_scl, scales_mode=mode, jitter=h_jit, jitter_mode=3)
    if ks:
        mo = scored_offset(torch.from_numpy(mh), torch.from_numpy(mo), jf, jt, kernel_size=ks).numpy()
    rs, ri, _, _ = oracle.nms_topk(oracle.bicubic4(mh), K)          # pinned by tests/test_oracle_golden.py and test_gpu_parity.py
    ref = oracle.collect_limbs(rs, ri, mo, True, hw, sk, pc.THRE, pc.MIN_LEN,
                               scales_hr=(oracle.bicubic4 if mode == 2 else oracle.bilinear4)(np.ascontiguousarray(ms)) if heads else None,
                               jitter_hr=oracle.bilinear4(np.ascontiguousarray(mj)) if heads else None)
    got, sc, ix = run(sk, n, hw, K, dev, **fields)
    assert (sc == rs).all() and (ix == ri).all()
    assert_limbs_match(ref, got, SCORE_TOL, valid_only_thre=pc.THRE)
    assert ((ref[..., 2] >= pc.THRE) & (ref[..., 5] >= pc.THRE)).mean() >= 0.25


# ---------------------------------------------------------------------------------- the collect fallback of og_generate_limbs_f32
@pytest.mark.parametrize("name", FALLBACK)
def test_fallback_hand_off(dev, name):
    """Both sides of the switch (pairing_cases.plan): a launch that returns the lists and one that keeps them in the workspace --
    where the collect fallback reads them back, [tickets | top-k | inds | scores] -- give the same limbs, the lists are the oracle's
    in either place, and a second launch on the warm workspace gives the same bytes."""
    case, scene, exp = pc.load(name)
    sk, n, hw, lib = pc.skeleton(case), pc.N_IMAGES, (case.H, case.W), _lib.load()
    assert pc.plan(n, 17, case.H, case.W, case.K).route == ('in_launch' if case.K == pc.IN_LAUNCH_K else 'fallback')
    rs, ri, _, _ = oracle.nms_topk(scene['hm_hr'], case.K)
    for o_tag, offs in offset_routes(scene):
        ws = torch.zeros(lib.og_generate_limbs_workspace_bytes(n, 17, case.H, case.W, case.K), dtype=torch.uint8, device=dev)
        runs = [run(sk, n, hw, case.K, dev, hmps=scene['hm_hr'], **offs),
                run(sk, n, hw, case.K, dev, hmps=scene['hm_hr'], own=True, ws=ws, **offs),
                run(sk, n, hw, case.K, dev, hmps=scene['hm_hr'], own=True, ws=ws, **offs),      # warm
                run(sk, n, hw, case.K, dev, hmps=scene['hm_hr'], ws=ws, **offs)]                # warm, the lists returned
        for got, sc, ix in runs:
            assert (sc == rs).all() and (ix == ri).all(), o_tag
            assert got.tobytes() == runs[0][0].tobytes(), o_tag
        assert_limbs_match(exp['limbs'], runs[0][0], SCORE_TOL)


def test_refusals_past_the_fallback(dev):
    """What the two entry points turn away, each with OG_EUNSUPPORTED before the pairing runs: the flip-folded form at a K that takes the
    fallback (the message names k), the jitter head with 4-component offsets, and every K past 2048 -- og_generate_limbs_f32 has no
    plan for it (no plane takes k > 1888), og_collect_limbs_f32 has no launch."""
    case, scene, exp = pc.load(f'fallback_k{pc.FALLBACK_K}')
    sk, n = pc.skeleton(case), pc.N_IMAGES
    _, perm, _, keep = flip_tables(sk)
    pair = np.concatenate([scene['off_lr'], mirrored(scene['off_lr'], perm)])
    with pytest.raises(_lib.OgError, match=f'k = {case.K} is too large for the merge-and-pair stage of the flip-folded form') as e:
        run(sk, n, (case.H, case.W), case.K, dev, hmps=scene['hm_hr'], offs=pair, off_lowres=1, limb_perm=_lib.int_table(perm, dev),
            reserve_mask=_lib.int_table(keep, dev))
    assert e.value.code == _lib.OG_EUNSUPPORTED
    z = np.zeros((n, 17, 64, 64), np.float32)
    for nd, lists in ((4, None), (4, (np.zeros((n, 17, 8), np.float32), np.zeros((n, 17, 8), np.int64)))):
        with pytest.raises(_lib.OgError, match='square inputs, 2-component offsets') as e:
            run(sk, n, (64, 64), 8, dev, nd, lists=lists, hmps=z, offs=np.zeros((n, 4 * len(sk), 16, 16), np.float32), off_lowres=1,
                jitter=np.zeros((n, 2, 16, 16), np.float32), jitter_mode=3)
        assert e.value.code == _lib.OG_EUNSUPPORTED
    k = 2049
    assert _lib.load().og_generate_limbs_workspace_bytes(n, 17, 516, 516, k) == 0 and pc.plan(n, 17, 516, 516, k).route is None
    with pytest.raises(_lib.OgError, match=f'k={k} too large') as e:
        run(sk, n, (516, 516), k, dev, lists=(np.zeros((n, 17, k), np.float32), np.zeros((n, 17, k), np.int64)),
            offs=np.zeros((n, 2 * len(sk), 129, 129), np.float32), off_lowres=1)
    assert e.value.code == _lib.OG_EUNSUPPORTED


# ---------------------------------------------------------------------------------- directed maps over bump heat maps, every row
def bump_maps(case):
    """stride-4 bump heat maps of the case's size, [images | other images]"""
    return pc.bump_heatmaps(case.K, case.H // 4, case.W // 4)


def lowres_heads(case, scl, jit, mode=2):
    """descriptor fields of the stride-4 heads (hm_lowres admits no others), and the maps the oracle pairs on"""
    fields, hr = {}, {}
    if case.heads in ('scale', 'both'):
        fields.update(scales=scl, scales_mode=mode)
        hr.update(scales_hr=(oracle.bicubic4 if mode == 2 else oracle.bilinear4)(np.ascontiguousarray(scl[:pc.N_IMAGES])))
    if case.heads in ('jitter', 'both'):
        fields.update(jitter=jit, jitter_mode=3)
        hr.update(jitter_hr=oracle.bilinear4(np.ascontiguousarray(jit[:pc.N_IMAGES])))
    return fields, hr


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("name", ['plain_k7', 'plain_k33', 'plain_k65', 'both_k33'])
def test_scored_offsets_refined_inside_the_generate_launch(dev, name, ks):
    """ScoredArgs in the merge-and-pair launch (int indices from LDS).  score_ksize needs the stride-4 heat maps, which are then the
    source of the peaks too, so the planted hi-res peaks cannot be used: the case's directed offset / scale / jitter maps (guide
    points in (-1, 0) and past the image, the zero-offset limb) over bump heat maps.  Expected: the oracle's lists of the x4 bicubic
    maps and its pairing on offsets refined by the CPU formulation of scored_offset -- every row, sub-threshold ends included."""
    case, scene, _ = pc.load(name)
    sk, n, hw = pc.skeleton(case), pc.N_IMAGES, (case.H, case.W)
    jf, jt = [a for a, _ in sk], [b for _, b in sk]
    hm = np.ascontiguousarray(bump_maps(case)[:n])
    refined = scored_offset(torch.from_numpy(hm), torch.from_numpy(scene['off_lr']), jf, jt, kernel_size=ks).numpy()
    fields, hr = lowres_heads(case, scene['scl_lr'], scene['jit_lr'])
    rs, ri, _, _ = oracle.nms_topk(oracle.bicubic4(hm), case.K)
    ref = oracle.collect_limbs(rs, ri, refined, True, hw, sk, pc.THRE, pc.MIN_LEN, **hr)
    plain = oracle.collect_limbs(rs, ri, scene['off_lr'], True, hw, sk, pc.THRE, pc.MIN_LEN, **hr)
    assert (ref[..., 8] != plain[..., 8]).any(), "the refinement is meant to move guide points"
    got, sc, ix = run(sk, n, hw, case.K, dev, hmps=hm, hm_lowres=1, offs=scene['off_lr'], off_lowres=1, score_ksize=ks, **fields)
    assert (sc == rs).all() and (ix == ri).all()
    assert_limbs_match(ref, got, SCORE_TOL)
    assert (case.K < 65 or (ref[..., 2] < pc.THRE).any()) and ((ref[..., 2] >= pc.THRE) & (ref[..., 5] >= pc.THRE)).mean() >= 0.25


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("perturbed", [False, True])
@pytest.mark.parametrize("name", ['both_k33', 'scale_k33'])
def test_flip_heads_on_mirrored_pairs(dev, name, perturbed, mode):
    """FlipHeadsArgs on [images | mirrored images] built from a case's directed offset / scale / jitter maps over bump heat maps (a
    planted stride-4 cell upsamples to a plateau of equal pixels, so the planted peaks cannot be kept).  The exact mirror -- planes and
    limbs permuted, flipped along W, x negated -- merges back to the un-mirrored maps: expected is the oracle's pairing on THOSE, no
    merge involved.  With a dyadic perturbation on the mirrored offsets and heads: the pairing on oracle.flip_merge's maps and the
    merged heads.  Every row, sub-threshold ends included."""
    case, scene, _ = pc.load(name)
    sk, n, hw = pc.skeleton(case), pc.N_IMAGES, (case.H, case.W)
    kp, perm, reserve, keep = flip_tables(sk)
    hm, off, scl, jit = np.ascontiguousarray(bump_maps(case)[:n]), scene['off_lr'], scene['scl_lr'], scene['jit_lr']
    flipped = lambda a: np.ascontiguousarray(a[..., ::-1])  # noqa: E731
    hm_m, scl_m, off_m = np.empty_like(hm), np.empty_like(scl), mirrored(off, perm)
    hm_m[:, list(kp)], scl_m[:, list(kp)] = flipped(hm), flipped(scl)
    jit_m = None
    if jit is not None:
        jit_m = flipped(jit)
        jit_m[:, 0] *= np.float32(-1)
    if perturbed:
        off_m = off_m + pc._dyadic(56 + case.K, off_m.shape, -48, 47, 4)
        scl_m = scl_m + pc._dyadic(57 + case.K, scl_m.shape, 0, 63, 4)
        jit_m = jit_m + pc._dyadic(58 + case.K, jit_m.shape, -16, 15, 8) if jit is not None else None
    pair = lambda a, b: np.concatenate([a, b])  # noqa: E731
    mh, mo = oracle.flip_merge(pair(hm, hm_m), pair(off, off_m), kp, perm, reserve)
    ms = (scl + flipped(scl_m[:, list(kp)])) / np.float32(2)
    mj = None
    if jit is not None:
        back = flipped(jit_m)
        back[:, 0] *= np.float32(-1)
        mj = (jit + back) / np.float32(2)
    assert (mh == hm).all()
    if not perturbed:
        assert (mo == off).all() and (ms == scl).all() and (mj is None or (mj == jit).all())
        mo, ms, mj = off, scl, jit
    fields, _ = lowres_heads(case, pair(scl, scl_m), pair(jit, jit_m) if jit is not None else None, mode)
    _, hr = lowres_heads(case, ms, mj, mode)
    rs, ri, _, _ = oracle.nms_topk(oracle.bicubic4(hm), case.K)
    ref = oracle.collect_limbs(rs, ri, mo, True, hw, sk, pc.THRE, pc.MIN_LEN, **hr)
    if perturbed:
        un = oracle.collect_limbs(rs, ri, off, True, hw, sk, pc.THRE, pc.MIN_LEN, **lowres_heads(case, scl, jit, mode)[1])
        assert (ref[..., 8] != un[..., 8]).any() and (ref[..., 11] != un[..., 11]).any(), "the perturbation is meant to show"
    got, sc, ix = run(sk, n, hw, case.K, dev, hmps=pair(hm, hm_m), hm_lowres=1, offs=pair(off, off_m), off_lowres=1,
                      kp_perm=_lib.int_table(kp, dev), limb_perm=_lib.int_table(perm, dev), reserve_mask=_lib.int_table(keep, dev), **fields)
    assert (sc == rs).all() and (ix == ri).all()
    assert_limbs_match(ref, got, SCORE_TOL)
