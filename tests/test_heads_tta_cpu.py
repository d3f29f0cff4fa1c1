"""CPU-only: the host side of the keypoint-scale / jitter heads under flip-test and --test-scales -- argument validation of the new C
entry points, merge_scales' checks and the nesting it returns, and the float32 numpy restatement of og_scale_accumulate_heads_f32 that
tests/test_gpu_heads_tta.py holds the kernel to (its own identity and unit cases are checked here)."""
import ctypes

import numpy as np
import pytest
import torch

from offsetguided_amd import _lib
from offsetguided_amd.config import coco_data as cd
from offsetguided_amd.decoder import multiscale

F32 = np.float32


# ---------------------------------------------------------------------------------- numpy restatement
def np_flip_heads(scl, jit, kp_perm=None):
    """og_flip_merge_heads_f32 restated (reference decoder/factory.py:108-113, :141-144): (2N, ...) pairs -> (N, ...), (a + b) / 2."""
    kp_perm = cd.heatmap_hflip(cd.COCO_KEYPOINTS) if kp_perm is None else kp_perm
    so = jo = None
    if scl is not None:
        scl = np.asarray(scl, F32)
        n = scl.shape[0] // 2
        so = (scl[:n] + scl[n:, :, :, ::-1][:, kp_perm]) / F32(2)
    if jit is not None:
        jit = np.asarray(jit, F32)
        n = jit.shape[0] // 2
        fl = jit[n:, :, :, ::-1].copy()
        fl[:, 0::2] *= F32(-1)
        jo = (jit[:n] + fl) / F32(2)
    return so, jo


def np_resample_plane(src, aff_row, h, w):
    """(P, hs, ws) planes of one image onto the (h, w) base grid: the operation order of csrc/scale_merge.hip, fp32 throughout."""
    _, hs, ws = src.shape
    Ax, Bx, Ay, By = [F32(v) for v in aff_row[:4]]
    u = Ax * np.arange(w, dtype=F32)
    u = np.minimum(np.maximum(u + Bx, F32(0)), F32(ws - 1))
    r = Ay * np.arange(h, dtype=F32)
    r = np.minimum(np.maximum(r + By, F32(0)), F32(hs - 1))
    x0, y0 = np.floor(u).astype(np.int64), np.floor(r).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    fx, fy = u - x0.astype(F32), (r - y0.astype(F32))[:, None]
    gx, gy = F32(1) - fx, F32(1) - fy
    p00, p01 = src[:, y0[:, None], x0[None, :]], src[:, y0[:, None], x1[None, :]]
    p10, p11 = src[:, y1[:, None], x0[None, :]], src[:, y1[:, None], x1[None, :]]
    top = p00 * gx + p01 * fx
    bot = p10 * gx + p11 * fx
    return (top * gy + bot * fy).astype(F32)


def np_resample_heads(scl, jit, aff, h, w):
    """One scale's (merged) scale maps (N, C, hs, ws) / jitter maps (N, 2, hs, ws) on the base grid, in base units: jitter channel 0 / 1
    times inv_ax / inv_ay, keypoint scales times sqrt(inv_ax * inv_ay) (one fp32 multiply, one correctly rounded fp32 square root)."""
    so = jo = None
    if scl is not None:
        so = np.empty(scl.shape[:2] + (h, w), F32)
        for n in range(scl.shape[0]):
            area = F32(aff[n][4]) * F32(aff[n][5])
            so[n] = np_resample_plane(scl[n], aff[n], h, w) * np.sqrt(area, dtype=F32)
    if jit is not None:
        jo = np.empty(jit.shape[:2] + (h, w), F32)
        for n in range(jit.shape[0]):
            jo[n] = np_resample_plane(jit[n], aff[n], h, w)
            jo[n, 0] *= F32(aff[n][4])
            jo[n, 1] *= F32(aff[n][5])
    return so, jo


def np_merge_heads(per_scale, affs, h, w, flip, last_scales=True):
    """The heads' part of merge_scales restated: per scale (scl | None, jit | None), flip pair merged first, resampled, summed in list
    order, times 1/S at the last scale (last_scales=False: the plain sum, what MODE_ADD alone leaves)."""
    S = len(per_scale)
    inv = F32(1) / F32(S)
    acc = None
    for s, ((scl, jit), aff) in enumerate(zip(per_scale, affs)):
        if flip:
            scl, jit = np_flip_heads(scl, jit)
        v = np_resample_heads(None if scl is None else np.asarray(scl, F32), None if jit is None else np.asarray(jit, F32), aff, h, w)
        if s == 0:
            acc = [None if a is None else a.copy() for a in v]
        else:
            acc = [None if a is None else a + b for a, b in zip(acc, v)]
            if s == S - 1 and last_scales:
                acc = [None if a is None else a * inv for a in acc]
    return acc


IDENTITY = np.array([[1, 0, 1, 0, 1, 1]], F32)


@pytest.mark.parametrize("flip", [False, True])
def test_restatement_identity(flip):
    """The restatement's own identity case: the table (1, 0, 1, 0, 1, 1) returns its (flip-merged) input bit for bit."""
    rng = np.random.default_rng(3)
    N, h, w = 2, 9, 13
    scl = rng.standard_normal(((2 if flip else 1) * N, 17, h, w)).astype(F32)
    jit = rng.standard_normal(((2 if flip else 1) * N, 2, h, w)).astype(F32)
    so, jo = np_merge_heads([(scl, jit)], [np.repeat(IDENTITY, N, 0)], h, w, flip)
    es, ej = np_flip_heads(scl, jit) if flip else (scl, jit)
    assert np.array_equal(so, es) and np.array_equal(jo, ej)


def test_restatement_flip_merge_is_the_torch_expression():
    """np_flip_heads == the reference's torch ops (decoder/factory.py:108-113, :141-144), bit for bit."""
    g = torch.Generator().manual_seed(5)
    scl, jit = torch.randn(4, 17, 6, 7, generator=g), torch.randn(4, 2, 6, 7, generator=g)
    perm = cd.heatmap_hflip(cd.COCO_KEYPOINTS)
    fl = torch.flip(jit[2:], [-1])
    fl[:, ::2] *= -1
    ej = (jit[:2] + fl) / 2
    es = (scl[:2] + torch.flip(scl[2:], [-1])[:, perm]) / 2
    so, jo = np_flip_heads(scl.numpy(), jit.numpy())
    assert np.array_equal(so, es.numpy()) and np.array_equal(jo, ej.numpy())


def test_restatement_units():
    aff = np.array([[2, 0, 4, 0, 0.5, 0.125]], F32)
    scl, jit = np.full((1, 17, 16, 8), 12, F32), np.empty((1, 2, 16, 8), F32)
    jit[:, 0], jit[:, 1] = 3.0, -5.0
    so, jo = np_resample_heads(scl, jit, aff, 4, 4)
    assert (so == 3.0).all() and (jo[:, 0] == 1.5).all() and (jo[:, 1] == -0.625).all()     # sqrt(1/16) = 1/4


# ---------------------------------------------------------------------------------- C entry points: validation without a GPU
def test_new_entry_points_validate_their_arguments():
    lib = _lib.load()
    one = ctypes.c_void_p(16)      # never dereferenced: every call below is refused before a launch
    rc = lib.og_flip_merge_heads_f32(None, None, 1, 17, 8, 8, None, None, None, None)
    assert rc == _lib.OG_EINVAL and b"neither head" in lib.og_last_error()
    rc = lib.og_flip_merge_heads_f32(one, None, 1, 17, 8, 8, one, None, None, None)
    assert rc == _lib.OG_EINVAL and b"output" in lib.og_last_error()
    rc = lib.og_flip_merge_heads_f32(one, None, 1, 17, 8, 8, None, one, None, None)
    assert rc == _lib.OG_EINVAL and b"kp_perm" in lib.og_last_error()
    rc = lib.og_flip_merge_heads_f32(None, one, 0, 17, 8, 8, None, None, one, None)
    assert rc == _lib.OG_EINVAL and b"bad shape" in lib.og_last_error()
    rc = lib.og_hmp_nms_k_f32(None, 1, 8, 8, 5, None, None)
    assert rc == _lib.OG_EINVAL and b"null pointer" in lib.og_last_error()
    for k in (0, 4, 9):
        rc = lib.og_hmp_nms_k_f32(one, 1, 8, 8, k, one, None)
        assert rc == _lib.OG_EUNSUPPORTED and b"window" in lib.og_last_error()
    rc = lib.og_scale_accumulate_heads_f32(one, one, one, None, 1, 0, 17, 19, 8, 8, None, None, None, one, 8, 8, 0, 1.0, one, one, None, None,
                                           None)
    assert rc == _lib.OG_EINVAL and b"accumulator" in lib.og_last_error()
    rc = lib.og_scale_accumulate_heads_f32(one, one, one, None, 1, 1, 17, 19, 8, 8, None, None, None, one, 8, 8, 0, 1.0, one, one, one, None,
                                           None)
    assert rc == _lib.OG_EINVAL and b"flip tables" in lib.og_last_error()
    rc = lib.og_scale_accumulate_heads_f32(one, one, None, one, 1, 0, 17, 19, 8, 8, None, None, None, one, 8, 8, 3, 1.0, one, one, None, one,
                                           None)
    assert rc == _lib.OG_EINVAL and b"mode" in lib.og_last_error()


def limbs_refusal(collect=False, **fields):
    """og_generate_limbs_f32 (or og_collect_limbs_f32) on the folded K1-fused flip form at 64 x 64 with `fields` changed -> (code, message)"""
    lib, one = _lib.load(), ctypes.c_void_p(16)      # never dereferenced
    form = dict(hmps=one, hm_lowres=1, kp_perm=one, offs=one, off_lowres=1, vector_nd=2, limb_perm=one, reserve_mask=one, N=1, C=17, H=64,
                W=64, jf=one, jt=one, L=19, k=8, thre_hmp=0.1, min_len=0.5, resize_factor=1.0, limbs=one)
    d = _lib.LimbsDesc(**dict(form, **fields))
    rc = lib.og_collect_limbs_f32(one, one, d, None) if collect else lib.og_generate_limbs_f32(d, one, 1 << 20, None)
    return rc, lib.og_last_error()


def test_flip_heads_form_validates_its_arguments():
    """What og_generate_limbs_fused_flip_heads_f32 refused, through the descriptor (its `neither head` refusal went with it: that
    combination is the flip form)."""
    rc, msg = limbs_refusal(score_ksize=2, scales=ctypes.c_void_p(16), scales_mode=2)
    assert rc == _lib.OG_EINVAL and b"ksize" in msg
    rc, msg = limbs_refusal(scales=ctypes.c_void_p(16), scales_mode=1)
    assert rc == _lib.OG_EINVAL and b"scales_mode" in msg
    rc, msg = limbs_refusal(kp_perm=None, scales=ctypes.c_void_p(16), scales_mode=2)
    assert rc == _lib.OG_EINVAL and b"null pointer" in msg
    # the jitter head keeps the square-input restriction of decoder/collect.py:158
    rc, msg = limbs_refusal(W=96, jitter=ctypes.c_void_p(16), jitter_mode=3)
    assert rc == _lib.OG_EUNSUPPORTED and b"square" in msg


NOFLIP = dict(kp_perm=None, limb_perm=None, reserve_mask=None)
ONE = ctypes.c_void_p(16)


@pytest.mark.parametrize("fields,code,text", [
    (dict(hm_lowres=0), _lib.OG_EUNSUPPORTED, b"kp_perm folds the stride-4 heat maps"),                  # kp_perm without hm_lowres
    (dict(limb_perm=None), _lib.OG_EINVAL, b"null pointer"),                                             # kp_perm without limb_perm
    (dict(reserve_mask=None), _lib.OG_EINVAL, b"null pointer"),                                          # limb_perm without reserve_mask
    (dict(limb_perm=None, kp_perm=None), _lib.OG_EINVAL, b"null pointer"),                               # reserve_mask without limb_perm
    (dict(vector_nd=4), _lib.OG_EUNSUPPORTED, b"flip fold needs the stride-4 offsets and 2 components"),
    (dict(off_lowres=0), _lib.OG_EUNSUPPORTED, b"flip fold needs the stride-4 offsets and 2 components"),
    (dict(NOFLIP, hm_lowres=0, score_ksize=3), _lib.OG_EUNSUPPORTED, b"scored offsets need the stride-4 maps"),   # hi-res heat maps
    (dict(NOFLIP, off_lowres=0, score_ksize=3), _lib.OG_EUNSUPPORTED, b"scored offsets need the stride-4 maps"),
    (dict(NOFLIP, vector_nd=4, score_ksize=3), _lib.OG_EUNSUPPORTED, b"2-component offsets"),
    (dict(score_ksize=4), _lib.OG_EINVAL, b"ksize"),
    (dict(score_ksize=9), _lib.OG_EINVAL, b"ksize"),
    (dict(score_ksize=-1), _lib.OG_EINVAL, b"ksize"),
    (dict(hm_lowres=0, kp_perm=None, scales=ONE, scales_mode=2), _lib.OG_EUNSUPPORTED, b"only with hm_lowres"),   # flip + scale map, hi-res
    (dict(hm_lowres=0, kp_perm=None, jitter=ONE, jitter_mode=3), _lib.OG_EUNSUPPORTED, b"only with hm_lowres"),
    (dict(NOFLIP, scales=ONE, scales_mode=1), _lib.OG_EINVAL, b"scales_mode"),                            # hm_lowres with hi-res scale maps
    (dict(NOFLIP, jitter=ONE, jitter_mode=1), _lib.OG_EINVAL, b"jitter_mode"),
    (dict(NOFLIP, scales=ONE), _lib.OG_EINVAL, b"scales_mode"),                                           # a map without its mode
    (dict(NOFLIP, scales_mode=4, scales=ONE), _lib.OG_EINVAL, b"scales_mode"),
    (dict(NOFLIP, jitter=ONE, jitter_mode=2), _lib.OG_EINVAL, b"jitter_mode"),
    (dict(NOFLIP, H=48, jitter=ONE, jitter_mode=3), _lib.OG_EUNSUPPORTED, b"square"),
    (dict(NOFLIP, vector_nd=4, jitter=ONE, jitter_mode=3), _lib.OG_EUNSUPPORTED, b"square"),
    (dict(NOFLIP, vector_nd=3), _lib.OG_EUNSUPPORTED, b"vector_nd"),
    (dict(H=62), _lib.OG_EINVAL, b"multiples of 4"),
    (dict(NOFLIP, hm_lowres=0, W=66), _lib.OG_EINVAL, b"multiples of 4"),                                # stride-4 offsets alone need it too
    (dict(NOFLIP, H=1 << 16), _lib.OG_EINVAL, b"bad shape"),                                              # H / 4 < 2^14
    (dict(L=0), _lib.OG_EINVAL, b"bad shape"),
    (dict(hmps=None), _lib.OG_EINVAL, b"null pointer"),
    (dict(limbs=None), _lib.OG_EINVAL, b"null pointer"),
    (dict(topk_scores=ONE), _lib.OG_EINVAL, b"go together"),
    (dict(H=8, W=8, k=40), _lib.OG_EINVAL, b"plane border"),
])
def test_limbs_descriptor_support_matrix(fields, code, text):
    """One refusal per rule of validate_limbs_desc (csrc/nms_topk.hip), each from the accepted folded flip form with one thing changed."""
    rc, msg = limbs_refusal(**fields)
    assert rc == code and text in msg and b"og_generate_limbs_f32:" in msg, (rc, msg)


def test_limbs_descriptor_collect_entry():
    """og_collect_limbs_f32 on the same descriptor: no flip fold, heat maps only for scored_off, no top-k stage to size k against."""
    rc, msg = limbs_refusal(collect=True)
    assert rc == _lib.OG_EUNSUPPORTED and b"og_collect_limbs_f32: the flip fold belongs to og_generate_limbs_f32" in msg
    rc, msg = limbs_refusal(collect=True, **dict(NOFLIP, hmps=None, score_ksize=3))
    assert rc == _lib.OG_EINVAL and b"null pointer" in msg
    rc, msg = limbs_refusal(collect=True, **dict(NOFLIP, vector_nd=3))
    assert rc == _lib.OG_EUNSUPPORTED and b"vector_nd" in msg
    rc, msg = limbs_refusal(collect=True, **dict(NOFLIP, hmps=None, k=4096))       # past every rule of the descriptor: the launch's own limit
    assert rc == _lib.OG_EUNSUPPORTED and b"too large" in msg
    lib = _lib.load()
    rc = lib.og_collect_limbs_f32(None, ONE, _lib.LimbsDesc(), None)
    assert rc == _lib.OG_EINVAL and b"null pointer" in lib.og_last_error()


# ---------------------------------------------------------------------------------- merge_scales: checks in front of the device
def test_merge_scales_rejects_inconsistent_heads():
    t = torch.zeros(1, 17, 4, 4)
    o = torch.zeros(1, 38, 4, 4)
    j = torch.zeros(1, 2, 4, 4)
    aff = [IDENTITY, IDENTITY]
    with pytest.raises(ValueError, match='same at every scale'):
        multiscale.merge_scales([(t, o, t, j), (t, o, t, None)], aff, False, base_hw=(4, 4))
    with pytest.raises(ValueError, match='same at every scale'):
        multiscale.merge_scales([(t, o), (t, o, None, j)], aff, False, base_hw=(4, 4))
    with pytest.raises(ValueError, match=r'\(hm, off\) or \(hm, off, scl, jit\)'):
        multiscale.merge_scales([(t, o, t), (t, o, t)], aff, False, base_hw=(4, 4))


def test_heads_reach_the_device_check_not_a_refusal():
    """4-tuples over several scales are served: on CPU tensors the first complaint is the device's (no NotImplementedError any more)."""
    t, o, j = torch.zeros(1, 17, 4, 4), torch.zeros(1, 38, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(_lib.OgError, match='GPU tensor'):
        multiscale.merge_scales([(t, o, t, j)] * 2, [IDENTITY] * 2, False, base_hw=(4, 4))


def test_merged_features_nesting():
    """Jitter in slot 2 of the heatmap tuple, scale in slot 2 of the offset tuple, as PostProcess.generate_limbs unpacks them."""
    hm, off, scl, jit = (torch.zeros(1, c, 2, 2) for c in (17, 38, 17, 2))
    f = multiscale.merged_features((hm, off, scl, jit), n_stacks=2)
    assert len(f[0][0]) == 2 and all(a is hm for a in f[0][0])
    assert all(a is jit for a in f[0][2]) and len(f[0][2]) == 2 and all(a is scl for a in f[1][2]) and len(f[1][2]) == 2
    assert f[0][1] == [[], []] and f[1][1] == [[], []] and all(a is off for a in f[1][0])
    f = multiscale.merged_features((hm, off, None, jit))
    assert f[0][2][-1] is jit and f[1][2] == [[]]
    f = multiscale.merged_features((hm, off))
    assert f[0][2] == [[]] and f[1][2] == [[]]


def test_accumulate_scale_wants_an_accumulator_per_head():
    t, o, j = torch.zeros(1, 17, 4, 4), torch.zeros(1, 38, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError, match='accumulator'):
        multiscale.accumulate_scale(t, o, IDENTITY, (t, o), 0, 1.0, False, scl=t, jit=j)
    with pytest.raises(ValueError, match='accumulator'):
        multiscale.accumulate_scale(t, o, IDENTITY, (t, o, t, j), 0, 1.0, False)
