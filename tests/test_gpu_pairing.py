"""The limb pairing (og_collect::limb_rows, csrc/collect_body.h) on the directed cases of tests/pairing_cases.py, every route that
accepts a case against the reference's stored output (tests/golden/pairing_edges.npz): og_collect_limbs_f32 on the stored lists
(int64 indices), og_generate_limbs_f32 on the planted heat maps (the in-launch pairing: int indices), offsets gathered from hi-res
maps / sampled from the stride-4 maps / flip-merged on load / refined on the spot (scored_off), the scale head in modes 1..3, the
jitter head in modes 1 and 3, 4-component offsets.  Both kernels run whole-wave groups: the half-wave GROUP = 32 variant the body's
comment speaks of is not instantiated in the library and is not tested here.  EXACT_LIMB_COLS bit for bit, the score within
SCORE_TOL, the returned lists equal to the stored ones.

The forms that start from stride-4 heat maps (fused, fused-flip, with heads, with scored_off) cannot have peaks planted exactly: they
run on bump scenes (pairing_cases.build_fused) against the oracle's lists and pairing, rows with both ends above the threshold."""
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
PLAIN = [c.name for c in pc.CASES if c.heads == 'none' and c.nd == 2 and c.skeleton == 'omp19']


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    _lib.load()
    return torch.device("cuda:0")


def run(sk, n, hw, k, dev, nd=2, lists=None, **form):
    """One call with the descriptor fields `form` (numpy arrays go to the device): og_collect_limbs_f32 on `lists` = (scores, inds),
    or og_generate_limbs_f32 -> limbs (N,L,k,13), returned scores, inds (None for the collect call), all numpy"""
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    form = {f: torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v for f, v in form.items()}
    limbs = torch.full((n, len(sk), k, 13), float('nan'), device=dev)
    d = _lib.LimbsDesc(N=n, C=17, H=hw[0], W=hw[1], jf=_lib.int_table([a for a, _ in sk], dev), jt=_lib.int_table([b for _, b in sk], dev),
                       L=len(sk), k=k, thre_hmp=pc.THRE, min_len=pc.MIN_LEN, resize_factor=1.0, limbs=limbs, vector_nd=nd, **form)
    if lists is not None:
        sc, ix = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in lists)
        _lib.check(lib.og_collect_limbs_f32(_lib.ptr(sc), _lib.ptr(ix), d, st), lib)
        return limbs.cpu().numpy(), None, None
    sc = torch.full((n, 17, k), float('nan'), device=dev)
    ix = torch.full((n, 17, k), -1, dtype=torch.int64, device=dev)
    d.topk_scores, d.topk_inds = sc.data_ptr(), ix.data_ptr()
    ws = torch.zeros(lib.og_generate_limbs_workspace_bytes(n, 17, hw[0], hw[1], k), dtype=torch.uint8, device=dev)
    _lib.check(lib.og_generate_limbs_f32(d, _lib.ptr(ws), ws.numel(), st), lib)
    out = limbs.cpu().numpy(), sc.cpu().numpy(), ix.cpu().numpy()
    assert int(ws[:61440].view(torch.int32).abs().sum()) == 0, "the reserved head of the workspace must stay zero"
    return out


def head_routes(case, scene, exp):
    """[(tag, descriptor fields of the head, expected limbs)]: every mode the case's head has"""
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


def check_coverage(case, scene, exp, ref):
    jit_hr = oracle.bilinear4(scene['jit_lr']) if scene['jit_lr'] is not None else None
    cnt = pc.counts(case, exp['scores'], exp['inds'], ref, oracle.bilinear4(scene['off_lr']), jit_hr)
    assert cnt and all(v >= 1 for v in cnt.values()), cnt


@pytest.mark.parametrize("name", NAMES)
def test_collect_on_the_stored_lists(dev, name):
    case, scene, exp = pc.load(name)
    sk = pc.skeleton(case)
    for h_tag, head, ref in head_routes(case, scene, exp):
        for o_tag, offs in offset_routes(scene):
            got, _, _ = run(sk, pc.N_IMAGES, (case.H, case.W), case.K, dev, case.nd, lists=(exp['scores'], exp['inds']), **offs, **head)
            assert not np.isnan(got).any(), (h_tag, o_tag)
            assert_limbs_match(ref, got, SCORE_TOL)
    check_coverage(case, scene, exp, ref)


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
    check_coverage(case, scene, exp, ref)


def weights(case):
    """stride-4 heat maps for scored_off to weigh with: dyadic, non-negative, a fifth of the cells zero"""
    w = pc._dyadic(77 + case.K, (pc.N_IMAGES, 17, case.H // 4, case.W // 4), -16, 63, 64)
    return np.maximum(w, 0).astype(np.float32)


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("name", PLAIN)
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
@pytest.mark.parametrize("name", PLAIN + ['plain44_k7'])
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
