"""Candidate limb collection (reference decoder/collect.py:21-273) on the HIP kernels K1+K2."""
import logging
import os

import torch

from .. import _lib
from ..config.coco_data import COCO_KEYPOINTS, COCO_PERSON_SKELETON
from .heatmap import _topk_raw

LOG = logging.getLogger(__name__)


class LimbsCollect(object):
    """Pairs top-k keypoint candidates into limbs along the guiding offsets.

    Same constructor and `generate_limbs` contract as the reference class
    (decoder/collect.py:37-67).  The output rows are
    [x1, y1, v1, x2, y2, v2, ind1, ind2, len_delta, len_limb, limb_score, scale1, scale2].
    Keypoint-scale and jitter-offset heads (off in every published configuration) are supported:
    K2 samples the stride-4 maps at the peaks with the arithmetic of F.interpolate(x4).

    The whole of generate_limbs -- NMS, top-k and the pairing -- is ONE C call: two launches queued back to back (band
    top-k; merge + pairing), on hi-res heatmaps (og_generate_limbs_f32) or straight on the stride-4 head output with the x4
    bicubic inside the band kernel (hm_lowres in the call's descriptor: K1-fused, the production path).
    """

    def __init__(self, hmp_s, off_s, *, topk=40, thre_hmp=0.08, min_len=3,
                 include_jitter_offset=False, include_scale=False, use_jitter_offset=True,
                 keypoints=COCO_KEYPOINTS, skeleton=COCO_PERSON_SKELETON):
        self.hmp_s = hmp_s
        self.off_s = off_s
        self.resize_factor = off_s / hmp_s
        self.keypoints = keypoints
        self.skeleton = skeleton
        self.K = topk
        self.thre_hmp = thre_hmp
        self.min_len = min_len
        self.include_jitter_offset = include_jitter_offset
        self.include_scale = include_scale
        self.use_jitter_offset = use_jitter_offset
        self.jtypes_f, self.jtypes_t = self.pack_jtypes(skeleton)
        self._desc_const = {}   # the constant part of the C call's descriptor per device and setting (_call)
        LOG.info('%d limbs, keypoint threshold %.4f, offset/heatmap unit ratio %.3f',
                 len(skeleton), thre_hmp, self.resize_factor)

    @staticmethod
    def pack_jtypes(skeleton):
        return [a for a, _ in skeleton], [b for _, b in skeleton]

    def _check_optional_heads(self, jomps_hr, scmps_hr, vector_nd):
        if vector_nd not in (2, 4):
            raise NotImplementedError('guiding offsets have 2 components, or 4 with cat_flip_offs')

    def _jitter(self, jomps):
        """The jitter maps only act when the head exists AND use_jitter_offset (collect.py:154, :212)."""
        return jomps if self.include_jitter_offset and self.use_jitter_offset and isinstance(jomps, torch.Tensor) else None

    def generate_limbs(self, hmps_hr, jomps_hr, offs_hr, scmps_hr, vector_nd=2):
        """(N,C,H,W) heatmaps + (N,2L,H,W) offsets at input resolution -> limbs (N,L,K,13)."""
        assert hmps_hr.shape[-2:] == offs_hr.shape[-2:], 'spatial resolution should be equal'
        self._check_optional_heads(jomps_hr, scmps_hr, vector_nd)
        scales = scmps_hr if self.include_scale and isinstance(scmps_hr, torch.Tensor) else None
        return self._collect(hmps_hr, offs_hr, off_is_lowres=False, vector_nd=vector_nd, scales=scales, scales_mode=1,
                             jitter=self._jitter(jomps_hr), jitter_mode=1)

    def generate_limbs_lowres(self, hmps_hr, offs_lr, vector_nd=2, scmps_lr=None, scale_inter='bicubic', jomps_lr=None):
        """Same result as generate_limbs(hmps_hr, [], F.interpolate(offs_lr, x4, 'bilinear'), [])
        without building the hi-res offset tensor: K2 samples it at the candidate peaks."""
        assert hmps_hr.shape[-2] == 4 * offs_lr.shape[-2] and hmps_hr.shape[-1] == 4 * offs_lr.shape[-1], \
            'spatial resolution should be equal'
        return self._collect(hmps_hr, offs_lr, off_is_lowres=True, vector_nd=vector_nd, scales=scmps_lr,
                             scales_mode=2 if scale_inter == 'bicubic' else 3, jitter=self._jitter(jomps_lr), jitter_mode=3)

    def generate_limbs_flip(self, hmps_hr, offs_pair_lr, limb_perm, reserve_mask):
        """generate_limbs_lowres on the flip-merged offsets WITHOUT merging them first: offs_pair_lr = the stride-4 offset head
        output for [images | mirrored images], (2N, 2L, h, w); every sampled tap is computed as PostProcess.flip_augment would
        have written it (decoder/factory.py:129-138).  2-component offsets, no scale / jitter head."""
        hmps_hr = _lib.require_device(hmps_hr, 'hmps_hr')
        offs = _lib.require_device(offs_pair_lr, 'offs')
        n, c, h, w = hmps_hr.shape
        assert tuple(offs.shape) == (2 * n, 2 * len(self.skeleton), h // 4, w // 4), 'offsets of [images | mirrored images] at stride 4'
        dev = hmps_hr.device
        return self._call('k1_generate_limbs', hmps_hr, offs, (n, c, h, w), off_lowres=1, vector_nd=2,
                          limb_perm=_lib.int_table(limb_perm, dev), reserve_mask=_lib.int_table(reserve_mask, dev))

    def generate_limbs_fused_flip(self, hm_pair_lr, offs_pair_lr, kp_perm, limb_perm, reserve_mask, scored_ks=0, scmps_pair_lr=None,
                                  scale_inter='bicubic', jomps_pair_lr=None):
        """generate_limbs_fused on the flip-merged maps WITHOUT merging them first (LimbsDesc.kp_perm / limb_perm): the stride-4
        head outputs of [images | mirrored images], (2N, C, h, w) and (2N, 2L, h, w); every heat-map source value and every offset tap
        is computed as PostProcess.flip_augment would have written it (decoder/factory.py:98-146).  2-component offsets.  scored_ks > 0:
        scored_off with that window, every offset tap refined inside the pairing (LimbsDesc.score_ksize); 0 = the unrefined call.
        scmps_pair_lr (2N, C, h, w) / jomps_pair_lr (2N, 2, h, w): the keypoint-scale / jitter head outputs of the same pairs, sampled
        at the peaks as flip_augment would have merged them (the jitter maps act under the conditions of _jitter and need square
        inputs, as everywhere)."""
        hm = _lib.require_device(hm_pair_lr, 'hmps')
        offs = _lib.require_device(offs_pair_lr, 'offs')
        n2, c, h, w = hm.shape
        n, dev = n2 // 2, hm.device
        assert n2 == 2 * n and tuple(offs.shape) == (n2, 2 * len(self.skeleton), h, w), 'head outputs of [images | mirrored images] at stride 4'
        scl, jit = self._heads(scmps_pair_lr, 2 if scale_inter == 'bicubic' else 3, self._jitter(jomps_pair_lr), 3, (n2, c, 4 * h, 4 * w))
        return self._call('k1f_fused_limbs', hm, offs, (n, c, 4 * h, 4 * w), hm_lowres=1, off_lowres=1, vector_nd=2,
                          kp_perm=_lib.int_table(kp_perm, dev), limb_perm=_lib.int_table(limb_perm, dev),
                          reserve_mask=_lib.int_table(reserve_mask, dev), score_ksize=int(scored_ks), **scl, **jit)

    def generate_limbs_fused(self, hmps_lr, offs_lr, vector_nd=2, scmps_lr=None, scale_inter='bicubic', jomps_lr=None, scored_ks=0):
        """Same limbs as generate_limbs(F.interpolate(hmps_lr, x4, 'bicubic'), [], F.interpolate(offs_lr, x4,
        'bilinear'), []) with NEITHER hi-res tensor built: K1-fused upsamples inside the NMS kernel.  scored_ks > 0: scored_off
        with that window, every offset tap refined inside the pairing (LimbsDesc.score_ksize); 0 = the unrefined call."""
        assert hmps_lr.shape[-2:] == offs_lr.shape[-2:], 'spatial resolution should be equal'
        if scored_ks and vector_nd != 2:
            raise NotImplementedError('scored_off needs 2-component offsets (the reference fails here as well)')
        return self._collect(hmps_lr, offs_lr, off_is_lowres=True, hm_is_lowres=True, vector_nd=vector_nd,
                             scales=scmps_lr, scales_mode=2 if scale_inter == 'bicubic' else 3,
                             jitter=self._jitter(jomps_lr), jitter_mode=3, scored_ks=scored_ks)

    def _collect(self, hmps_hr, offs, off_is_lowres, hm_is_lowres=False, vector_nd=2, scales=None, scales_mode=0,
                 jitter=None, jitter_mode=0, scored_ks=0):
        hmps_hr = _lib.require_device(hmps_hr, 'hmps_hr')
        offs = _lib.require_device(offs, 'offs')
        n, c, h, w = hmps_hr.shape
        if hm_is_lowres:
            h, w = 4 * h, 4 * w
        # cat_flip_offs hands the 4-component offsets on as a (2N, 2L, h, w) view (decoder/factory.py:127);
        # like collect.py:73 only the memory order (N, L, vector_nd, h, w) matters
        assert offs.numel() == n * vector_nd * len(self.skeleton) * offs.shape[-2] * offs.shape[-1], \
            'offset channels must be vector_nd x number of limbs'
        scl, jit = self._heads(scales, scales_mode, jitter, jitter_mode, (n, c, h, w))
        # one bracket round the whole generate_limbs boundary (K1 + K2): what bench.py prices as "K1"; K1-fused: the x4 bicubic runs
        # inside the NMS kernel
        return self._call('k1f_fused_limbs' if hm_is_lowres else 'k1_generate_limbs', hmps_hr, offs, (n, c, h, w),
                          hm_lowres=int(hm_is_lowres), off_lowres=int(off_is_lowres), vector_nd=int(vector_nd),
                          score_ksize=int(scored_ks), **scl, **jit)

    @staticmethod
    def _heads(scales, scales_mode, jitter, jitter_mode, nchw):
        """The optional heads as LimbsDesc fields ({} = head absent): maps at input resolution (mode 1) or the stride-4 head output."""
        n, c, h, w = nchw
        scl = jit = {}
        if scales is not None:   # keypoint-scale head (collect.py:111-122)
            scales = _lib.require_device(scales, 'scmps')
            expect = (n, c, h, w) if scales_mode == 1 else (n, c, h // 4, w // 4)
            assert tuple(scales.shape) == expect, f'scale maps {tuple(scales.shape)}, expected {expect}'
            scl = dict(scales=scales, scales_mode=int(scales_mode))
        if jitter is not None:   # jitter-offset head: two shared channels
            jitter = _lib.require_device(jitter, 'jomps')
            expect = (n, 2, h, w) if jitter_mode == 1 else (n, 2, h // 4, w // 4)
            assert tuple(jitter.shape) == expect, f'jitter maps {tuple(jitter.shape)}, expected {expect}'
            if h != w:   # the reference indexes the refinement maps [x][y] (collect.py:158-165)
                raise NotImplementedError('the jitter-offset head needs square inputs (the reference indexes its maps [x][y])')
            jit = dict(jitter=jitter, jitter_mode=int(jitter_mode))
        return scl, jit

    def _call(self, timer, hmps, offs, nchw, **form):
        """ONE og_generate_limbs_f32 call = two launches (band top-k; merge + pairing): nchw = images, joint channels and the INPUT
        resolution; form = the LimbsDesc fields that tell the forms apart (tensors for pointers).  The descriptor is a copy of the
        cached constant part with this call's fields written over it: the host path of the decoder's hot call."""
        dev, lib = hmps.device, _lib.load()
        const = (dev.index, len(self.skeleton), self.K, self.thre_hmp, self.min_len, self.resize_factor)
        if const not in self._desc_const:
            self._desc_const[const] = _lib.LimbsDesc(jf=_lib.int_table(self.jtypes_f, dev), jt=_lib.int_table(self.jtypes_t, dev),
                                                     **dict(zip(('L', 'k', 'thre_hmp', 'min_len', 'resize_factor'), const[1:])))
        desc = _lib.LimbsDesc.from_buffer_copy(self._desc_const[const])
        limbs = torch.empty((nchw[0], desc.L, desc.k, 13), dtype=torch.float32, device=dev)
        desc.N, desc.C, desc.H, desc.W = nchw
        desc.hmps, desc.offs, desc.limbs = hmps.data_ptr(), offs.data_ptr(), limbs.data_ptr()
        for name, v in form.items():    # an int, or a tensor for its pointer
            setattr(desc, name, v if type(v) is int else v.data_ptr())
        with _lib.stage_timer(timer, dev):
            ws = _lib.workspace(dev, lib.og_generate_limbs_workspace_bytes(*nchw, desc.k), 'limbs')   # zero-filled
            _lib.check(lib.og_generate_limbs_f32(desc, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)), lib)
        return limbs
