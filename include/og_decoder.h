/*
 * og_decoder.h -- C ABI of libog_decoder.so: the OffsetGuided decoder hot path as
 * hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (hellojialee/OffsetGuided) is pure Python: it has no native boundary of
 * its own.  Each entry point below replaces the torch-op sequence of one reference
 * function (file:line given per function, relative to the reference repository root); the
 * Python package offsetguided_amd.decoder binds them with ctypes behind the reference's own
 * names (hmp_NMS, topK_channel, joint_dets, LimbsCollect, GreedyGroup, PostProcess).
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - all tensor pointers are DEVICE pointers to dense, contiguous fp32 / int64 / int32 data
 *     in the reference's NCHW layout; nothing is copied or retained;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is
 *     stream-ordered, asynchronous, and performs no allocation and no host synchronisation
 *     (hipGraph-capturable); scratch comes from the caller through `workspace`;
 *   - return value: 0 on success, negative OG_E* code on failure; og_last_error() returns a
 *     thread-local message for the last failure on the calling thread; nothing throws;
 *   - inputs must be finite (NaN ordering of torch.topk is not reproduced);
 *   - no CPU fallback exists: without a HIP device every compute entry point fails.
 */
#ifndef OG_DECODER_H
#define OG_DECODER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OG_ABI_VERSION 4

#define OG_OK 0
#define OG_EINVAL (-1)    /* bad argument (shape, k, alignment, null pointer)        */
#define OG_ENOSPC (-2)    /* workspace too small                                     */
#define OG_EHIP (-3)      /* HIP runtime error (launch failure, no device)           */
#define OG_EUNSUPPORTED (-4)

int og_abi_version(void);
const char *og_last_error(void);

/* Number of HIP devices visible, or a negative OG_E* code. */
int og_device_count(void);

/* ---- a5: F.interpolate(hmps, scale_factor=4, mode='bicubic')  decoder/factory.py:74-75 ----
 * src (planes,h,w) -> dst (planes,4h,4w); torch-CPU fp32 arithmetic, bit-exact (A=-0.75,
 * align_corners=False, index-clamped taps). */
int og_upsample_bicubic4_f32(const float *src, long planes, int h, int w, float *dst, void *stream);

/* ---- a5: F.interpolate(offs, scale_factor=4, mode='bilinear')  decoder/factory.py:77-78 ----
 * Full materialisation; the decode path does not need it (og_collect_limbs_f32 samples the
 * low-res map at the peaks with the same arithmetic). */
int og_upsample_bilinear4_f32(const float *src, long planes, int h, int w, float *dst, void *stream);

/* ---- a6: hmp_NMS  decoder/heatmap.py:15-35 ----
 * out = heat * (maxpool3x3(zero-padded heat) == heat); heat/out (planes,H,W). */
int og_hmp_nms_f32(const float *heat, long planes, int H, int W, float *out, void *stream);

/* Same with another window: out = heat * (maxpool_kernel(zero-padded heat) == heat), kernel odd, 1..7 (OG_EUNSUPPORTED otherwise).
 * Exact compares; the zero padding takes part in the maximum; a suppressed element is heat * 0 (it keeps the sign of its input).
 * One launch, 64 x 16 tiles with their halo staged in LDS. */
int og_hmp_nms_k_f32(const float *heat, long planes, int H, int W, int kernel, float *out, void *stream);

/* ---- a7: topK_channel  decoder/heatmap.py:38-49 ----
 * Per-plane top-k of `scores` (planes, hw), sorted by value descending; ties: lower flat
 * index first (-0.0 == +0.0).  Outputs scores (planes,k) f32 and inds (planes,k) i64; the
 * caller derives ys = inds / w (floor) and xs = inds % w.
 * workspace: og_topk_workspace_bytes(planes, H, W, k). */
int og_topk_channel_f32(const float *scores, long planes, int H, int W, int k, float *out_scores,
                        int64_t *out_inds, void *workspace, size_t workspace_bytes, void *stream);

/* ---- a8: joint_dets = topK_channel(hmp_NMS(hmps), k)  decoder/heatmap.py:52-59 ----
 * Fused single pass over the hi-res heatmaps: the NMS map is never written.  Same outputs
 * and tie rule as og_topk_channel_f32 applied to og_hmp_nms_f32's result (zero-valued filler
 * entries, if a plane has fewer than k positive peaks, are the lowest flat indices whose NMS
 * value is zero).  Requires 2*(H+W)-4 >= k.
 * workspace: og_topk_workspace_bytes(planes, H, W, k). */
int og_nms_topk_f32(const float *hmps, long planes, int H, int W, int k, float *out_scores,
                    int64_t *out_inds, void *workspace, size_t workspace_bytes, void *stream);

/* ---- a5+a8 fused: joint_dets(F.interpolate(hmps, x4, 'bicubic'), k)  decoder/factory.py:74-75 + heatmap.py:52-59 ----
 * hmps_lr (planes,h,w) = stride-4 head output.  The (planes,4h,4w) hi-res heatmap is never
 * materialised: every band computes its hi-res rows on the fly (same rounding as
 * og_upsample_bicubic4_f32) and feeds them to the same NMS / top-k machinery.  Outputs, tie rule
 * and workspace exactly as og_nms_topk_f32 on the upsampled tensor (indices are hi-res flat
 * indices): workspace og_topk_workspace_bytes(planes, 4h, 4w, k). */
int og_upsample_nms_topk_f32(const float *hmps_lr, long planes, int h, int w, int k, float *out_scores,
                             int64_t *out_inds, void *workspace, size_t workspace_bytes, void *stream);

size_t og_topk_workspace_bytes(long planes, int H, int W, int k);

/* ---- a8+a9+a10: LimbsCollect.generate_limbs  decoder/collect.py:62-236 (+ _channel_dets :246-254) behind ONE descriptor ----
 * limbs (N,L,k,13) [x1,y1,v1,x2,y2,v2,ind1,ind2,min_dist,len,score,scale1,scale2].  Every form of the call is a setting of
 * OgLimbsDesc; which settings go together is checked in one place (validate_limbs_desc, csrc/nms_topk.hip).  The entry points of
 * ABI 3 (bench.py and the committed profiles still print their names) are these settings:
 *   og_generate_limbs_f32 (ABI 3)             hm_lowres 0, no perm; the reserved `flags` is gone
 *   og_generate_limbs_flip_f32                hm_lowres 0, off_lowres 1, vector_nd 2, limb_perm + reserve_mask
 *   og_generate_limbs_fused_f32               hm_lowres 1, off_lowres 1 (H, W = 4h, 4w)
 *   og_generate_limbs_fused_flip_f32          ... + kp_perm, limb_perm + reserve_mask, vector_nd 2
 *   og_generate_limbs_fused_scored_f32        og_generate_limbs_fused_f32 + score_ksize, vector_nd 2
 *   og_generate_limbs_fused_flip_scored_f32   og_generate_limbs_fused_flip_f32 + score_ksize
 *   og_generate_limbs_fused_flip_heads_f32    og_generate_limbs_fused_flip[_scored]_f32 + scales (mode 2 / 3) and / or jitter (mode 3)
 *   og_collect_limbs{,_nd,_ex,_full}_f32      og_collect_limbs_f32 with the same descriptor (hmps unused unless score_ksize) */
typedef struct OgLimbsDesc {
    uint32_t size;             /* sizeof(OgLimbsDesc): anything else is refused (OG_EINVAL, "descriptor size") */
    /* heat maps: hm_lowres 0 = (N,C,H,W) at input resolution; 1 = the stride-4 head output (N,C,H/4,W/4), the x4 bicubic of
     * decoder/factory.py:74-75 runs inside the band kernel (bit-identical to og_upsample_bicubic4_f32; K1-fused, the production path) */
    const float *hmps;
    int hm_lowres;
    /* flip-test fold of the heat maps (hm_lowres only): hmps (2N,C,H/4,W/4) = [images | mirrored images], every source value
     * (a + flipW(b)[kp_perm]) / 2 as og_flip_merge_f32 would have written it; int32[C] device array (config.heatmap_hflip) or NULL */
    const int32_t *kp_perm;
    /* guiding offsets: off_lowres 1 = (N,vector_nd*L,H/4,W/4) stride-4 head output, bilinearly sampled at the from-peaks exactly as
     * factory.py:77-78 + collect.py:143-147 would; 0 = (N,vector_nd*L,H,W), gathered.  vector_nd 2, or 4 = the `cat_flip_offs` form
     * (factory.py:115-127: offs from og_flip_cat_f32, match distance = the 4-D norm of (guide - to, guide' - to)) */
    const float *offs;
    int off_lowres;
    int vector_nd;
    /* flip-test fold of the offsets (both or neither; off_lowres, 2 components): offs (2N,2L,H/4,W/4) of [images | mirrored images],
     * every tap (a + flipW(b)[limb_perm]) / 2, x negated, the limbs of reserve_mask un-averaged; int32[L] device arrays
     * (config.offset_hflip).  og_generate_limbs_f32 only.  With hm_lowres the heat maps are folded as well (kp_perm) */
    const int32_t *limb_perm;
    const int32_t *reserve_mask;
    /* 0, or odd 1..7: scored_off (decoder/offset.py:8-43) inside the pairing -- every bilinear tap of the offset sampling is the refined
     * value of its stride-4 cell, computed on the spot from the (flip-merged-on-load) window of hmps, so the refined tensor is never
     * built; needs hm_lowres, off_lowres, 2 components.  Bit-identical to (og_flip_merge_f32 +) og_scored_offset_f32 in front */
    int score_ksize;
    /* keypoint-scale head (collect.py:111-122, :257-262): limbs columns 11 / 12 = the scale map of the from / to joint channel at the
     * from-peak / the matched to-peak instead of the constant 4.  scales_mode 0: no head (scales NULL); 1: (N,C,H,W), gathered; 2 / 3:
     * (N,C,H/4,W/4) = the head output, sampled as F.interpolate(x4, 'bicubic' / 'bilinear') would (factory.py:80-82) */
    const float *scales;
    int scales_mode;
    /* jitter-offset head (collect.py:127-138, :154-165, :210-214): (N,2,..) = the two shared refinement channels; jitter_mode 0: none;
     * 1: maps at input resolution; 3: stride-4 head output, sampled as F.interpolate(x4, 'bilinear') would (factory.py:84-88).  The guide
     * point is refined by the vector read at its truncated coordinates ([x][y] indexing of the reference: square inputs only) and the
     * limb's end points move by the vectors at their own peaks.  With hm_lowres only the stride-4 modes (scales 2 / 3, jitter 3); with the
     * flip fold (hm_lowres only) both maps are the (2N,..) pairs, every tap the value og_flip_merge_heads_f32 would have written -- a
     * kernel instantiation of its own, the other forms keep their registers and LDS */
    const float *jitter;
    int jitter_mode;
    int N, C, H, W;            /* images, joint channels, INPUT-resolution size (also with hm_lowres: the head output is H/4 x W/4) */
    const int32_t *jf;         /* device int32[L] from / to joint channel per limb (LimbsCollect.pack_jtypes) */
    const int32_t *jt;
    int L, k;
    float thre_hmp, min_len, resize_factor;
    /* outputs: the optional (N,C,k) lists of the joint_dets stage (both or neither; og_generate_limbs_f32 only) and the limbs */
    float *topk_scores;
    int64_t *topk_inds;
    float *limbs;
} OgLimbsDesc;

/* = og_nms_topk_f32 / og_upsample_nms_topk_f32 (joint_dets, decoder/heatmap.py:52-59) followed by og_collect_limbs_f32 on the same
 * descriptor, bit-identical limbs.  Two launches queued back to back -- band top-k, then ONE kernel that merges the band lists and
 * pairs the limbs.  Shapes whose merge-and-pair stage does not fit the LDS (large k) finish with og_collect_limbs_f32's kernel; with
 * the flip fold they are refused with OG_EUNSUPPORTED: take the unfolded route (og_flip_merge_f32 in front).
 * workspace: og_generate_limbs_workspace_bytes(N, C, H, W, k) bytes, 16-byte aligned, ZERO-FILLED by the caller (hipMemset) before its
 * first use; every call leaves it ready for the next one (any shape).  Its first 64 KiB are reserved and stay zero. */
int og_generate_limbs_f32(const OgLimbsDesc *d, void *workspace, size_t workspace_bytes, void *stream);

/* The pairing alone: scores / inds (N,C,k) from og_nms_topk_f32 on the (N,C,H,W) heat maps.  Reads d->hmps only with score_ksize (the
 * stride-4 heat maps the refinement weighs with); limb_perm is refused (OG_EUNSUPPORTED); topk_scores / topk_inds are ignored. */
int og_collect_limbs_f32(const float *scores, const int64_t *inds, const OgLimbsDesc *d, void *stream);

size_t og_generate_limbs_workspace_bytes(int N, int C, int H, int W, int k);

/* ---- flip-test without a merge pass: PostProcess.flip_augment (decoder/factory.py:98-146, the averaged form) folded into the
 * loads of its consumers (OgLimbsDesc.kp_perm / limb_perm above, and this one for the unfused route): hm_pair (2N,C,h,w) of
 * [images | mirrored images] -> dst (N,C,4h,4w), every value (a + flipW(b)[kp_perm]) / 2 exactly as og_flip_merge_f32 would have
 * written it; kp_perm int32[C] (config.heatmap_hflip).  Bit-identical to og_flip_merge_f32 + og_upsample_bicubic4_f32. */
int og_upsample_bicubic4_flip_f32(const float *hm_pair, const int32_t *kp_perm, int N, int C, int h, int w, float *dst, void *stream);

/* ---- a13: scored_offset  decoder/offset.py:8-43 (PostProcess: kernel_size 3, decoder/factory.py:70-72) ----
 * Heatmap-weighted offset refinement on the stride-4 maps: hm (N,C,h,w), off / out (N,2L,h,w) contiguous fp32, out must not alias off;
 * jf int32[L] device array, the start joint of every limb (pack_jtypes, 0-based).  Per limb l and component c
 *   out[n,2l+c] = box(hm[n,jf[l]] * off[n,2l+c]) / (box(hm[n,jf[l]]) + 1e-6f),
 * box = the sum over the ksize x ksize window clipped to the plane, with the rounding of the torch-CPU formulation: products rounded
 * before any sum (no FMA), both sums from +0 over the in-bounds cells row-major, one after the other; a correctly rounded divide.
 * Bit-identical to decoder.offset.scored_offset on CPU tensors.  ksize odd, 1..7 (anything else: OG_EINVAL).  One streaming launch
 * (LDS-tiled row bands, 16-byte accesses when w % 4 == 0 and the pointers are 16-byte aligned, a scalar path otherwise); no
 * allocation, no synchronisation, graph-capturable.  jf[l] in [0, C) is checked here when the table is host-visible (pinned) and is
 * the caller's duty otherwise, as for the other joint tables (a workgroup whose entry is out of range writes nothing).
 * OgLimbsDesc.score_ksize runs the same refinement inside the limb pairing. */
int og_scored_offset_f32(const float *hm, const float *off, int N, int C, int L, int h, int w, const int32_t *jf, int ksize,
                         float *out, void *stream);

/* ---- a12: GreedyGroup.group_skeletons  decoder/group.py:39-185 (+ :187-240) ----
 * One workgroup per image, device resident (replaces .cpu().numpy() + Pool.starmap,
 * decoder/factory.py:91-94).
 * limbs (N,L,k,13) -> poses (N,mmax,n_kp,6) [x,y,v,scale,limb_score,global_idx],
 * counts int32[N] = poses per image, status int32[N] = 0 ok / 1 subset table overflowed
 * (more than `mmax` partial skeletons alive; results for that image are then invalid).
 * Any skeleton / top-k: the partial-skeleton table and, for large L*k, the staged candidate rows move from LDS to the
 * workspace (L*k <= ~6 000 at mmax 128; OG_EUNSUPPORTED beyond).
 * workspace: og_group_workspace_bytes(N, L, k, n_kp, mmax). */
int og_greedy_group_f32(const float *limbs, int N, int L, int k, const int32_t *jf, const int32_t *jt,
                        int n_kp, double person_thre, float dist_max, int use_scale, int sort_dim, int mmax,
                        float *poses, int32_t *counts, int32_t *status, void *workspace, size_t workspace_bytes,
                        void *stream);

size_t og_group_workspace_bytes(int N, int L, int k, int n_kp, int mmax);

/* ---- a4: PostProcess.flip_augment (vector-addition form)  decoder/factory.py:98-146 ----
 * hm (2N,C,h,w), off (2N,2L,h,w) -> hm_out (N,C,h,w), off_out (N,2L,h,w).
 * kp_perm int32[C], limb_perm int32[L], reserve_mask int32[L] (1 = keep the un-averaged
 * original, config.offset_hflip()[1]) are device arrays. */
int og_flip_merge_f32(const float *hm, const float *off, int N, int C, int L, int h, int w,
                      const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask,
                      float *hm_out, float *off_out, void *stream);

/* ---- a4, the optional heads  decoder/factory.py:108-113 (jitter offsets), :141-144 (keypoint scales) ----
 * scmps (2N,C,h,w) -> sc_out (N,C,h,w) = (scmps[:N] + flipW(scmps[N:])[:, kp_perm]) / 2;
 * jomps (2N,2,h,w) -> jo_out (N,2,h,w) = (jomps[:N] + flipW(jomps[N:] with channel 0 = x negated)) / 2, no permutation.
 * Either head may be NULL together with its output (not both); kp_perm int32[C] device array, needed with scmps.  The sum is
 * taken first and halved after, bit-identical to the torch expressions above.  One launch for both maps. */
int og_flip_merge_heads_f32(const float *scmps, const float *jomps, int N, int C, int h, int w, const int32_t *kp_perm,
                            float *sc_out, float *jo_out, void *stream);

/* ---- a4, cat_flip_offs=True form  decoder/factory.py:115-127 ----
 * Same inputs; off_out (N,4L,h,w): per limb [x, y, mirrored x, mirrored y] (reserve limbs repeat x, y). */
int og_flip_cat_f32(const float *hm, const float *off, int N, int C, int L, int h, int w,
                    const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask,
                    float *hm_out, float *off_out, void *stream);

/* ---- multi-scale test: one scale's head outputs onto the base grid  (decoder/multiscale.py; beyond the reference) ----
 * hm (F*N,C,hs,ws), off (F*N,2L,hs,ws) of the scale, F = 2 with flip (the [images | mirrored images] pair, merged as
 * og_flip_merge_f32 merges it: kp_perm / limb_perm / reserve_mask as there, may be NULL without flip), F = 1 without.
 * aff (N,6) fp32 device table per image: Ax, Bx, Ay, By, inv_ax, inv_ay.  Base cell (j, i): u = Ax*j + Bx clamped to
 * [0, ws-1], x0 = floor(u), x1 = min(x0+1, ws-1), fx = u - x0 (rows alike); top = p00*(1-fx) + p01*fx, bot = p10*(1-fx) +
 * p11*fx, v = top*(1-fy) + bot*fy; offsets then v*inv_ax (x, even channels) / v*inv_ay (y, odd channels).
 * hm_acc (N,C,h,w), off_acc (N,2L,h,w): mode 0 writes v, 1 adds v, 2 adds v then multiplies by inv_count (the last scale).
 * The identity table (1, 0, 1, 0, 1, 1) reproduces the (merged) input.  One launch for both maps. */
int og_scale_accumulate_f32(const float *hm, const float *off, int N, int flip, int C, int L, int hs, int ws,
                            const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask,
                            const float *aff, int h, int w, int mode, float inv_count, float *hm_acc, float *off_acc,
                            void *stream);

/* Same launch over [hm | off | scl | jit]: scl (F*N,C,hs,ws) keypoint scales and / or jit (F*N,2,hs,ws) jitter offsets, each NULL
 * together with its accumulator scl_acc (N,C,h,w) / jit_acc (N,2,h,w).  With flip the pairs are merged as og_flip_merge_heads_f32
 * merges them, before the resample.  Units: a jitter offset is multiplied by inv_ax (channel 0) / inv_ay (channel 1) as the guiding
 * offsets are; a keypoint scale is a length in scale-s input pixels and is multiplied by sqrtf(inv_ax * inv_ay) (one fp32 multiply,
 * one correctly rounded square root).  Everything else, hm_acc / off_acc included, as og_scale_accumulate_f32. */
int og_scale_accumulate_heads_f32(const float *hm, const float *off, const float *scl, const float *jit, int N, int flip, int C,
                                  int L, int hs, int ws, const int32_t *kp_perm, const int32_t *limb_perm,
                                  const int32_t *reserve_mask, const float *aff, int h, int w, int mode, float inv_count,
                                  float *hm_acc, float *off_acc, float *scl_acc, float *jit_acc, void *stream);

/* ---- backbone epilogues (bf16, channels-last / NHWC activations of the inference engine) ----
 * Stand-alone epilogue / layout passes.  In the engine every convolution carries its epilogue itself (og_conv*_ below);
 * og_bias_act_* is what remains for a convolution that torch ran (InferenceEngine(strict=False) only), og_upsample2_add_* the
 * hourglass merge at the levels whose last convolution is not the tiled kernel.
 *
 * og_bias_act_bf16: x (pixels, channels) bf16, in place:  x = act(x + bias[c] (+ skip))
 *   = convolution.forward models/hourglass_104.py:26-30 (BN folded into bias, ReLU) and
 *     residual.forward :70-79 (bn2 + skip, ReLU).  bias fp32[channels]; skip bf16 like x or NULL;
 *     channels % 8 == 0; fp32 arithmetic, one rounding to bf16.
 * og_upsample2_add_bf16: up (n,H,W,channels) += nearest_x2(low (n,H/2,W/2,channels))
 *   = kp_module.forward :183-190 (up1 + up2 merge). */
int og_bias_act_bf16(void *x, const float *bias, const void *skip, long pixels, int channels, int relu, void *stream);
int og_upsample2_add_bf16(void *up, const void *low, long n, int H, int W, int channels, void *stream);

/* Engine boundary conversions (models/networks.py:189-194 hands fp32 NCHW in and out; the engine computes bf16 NHWC):
 * og_nchw_f32_to_nhwc_bf16: images (N,3,H,W) fp32 -> (N,H,W,3) bf16, one pass.
 * og_nhwc_bf16_to_nchw_f32: channels [first, first+channels) of src (N,H,W,src_channels) bf16, plus bias[first+c]
 *   (fp32[src_channels] or NULL), -> dst (N,channels,H,W) fp32: the head maps of models/heads.py:48-70,116-142 out of
 *   ONE 1x1 convolution that evaluates all heads. */
int og_nchw_f32_to_nhwc_bf16(const float *src, void *dst, long N, int C, int H, int W, void *stream);
int og_nhwc_bf16_to_nchw_f32(const void *src, int src_channels, int first_channel, int channels, const float *bias,
                             float *dst, long N, int H, int W, void *stream);

/* ---- evaluate.py input side (the rescale by cv2.resize is NOT included) ----
 * CenterPad + ToTensor + Normalize, transforms/pad.py:40-66 + evaluate.py:163-168: img (h,w,3) uint8 RGB on the device ->
 * out (3,target_h,target_w) fp32 = (px/255 - mean)/std with px the image pixel or `fill3` (124,116,104 in the
 * reference); mean3/std3/fill3 are HOST arrays of 3 floats; ltrb (host int[4], may be NULL) receives the paddings that
 * the annotations / annotations_inverse need. */
int og_center_pad_normalize_u8(const unsigned char *img, int h, int w, int target_h, int target_w, const float *mean3,
                               const float *std3, const float *fill3, float *out, int *ltrb, void *stream);

/* RescaleLongAbsolute's cv2.resize(INTER_CUBIC) (transforms/scale.py:27) for (h,w,3) uint8 images in HBM -> (new_h,new_w,3).
 * OpenCV's published 8-bit algorithm (fixed-point taps, replicated border); pinned bit-exactly to the CPU restatement
 * oracle/og_oracle.c:ogo_resize_cubic_u8 -- parity with cv2 itself is unpinned (third-party, absent from the build). */
int og_resize_cubic_u8(const unsigned char *src, int h, int w, unsigned char *dst, int new_h, int new_w, void *stream);

/* GT encoder input: the full-resolution uint8 mask_miss (N,h,w), 0 / 255, to the boolean mask at output
 * resolution -- cv2.resize(fx = fy = 1 / stride, INTER_CUBIC) / 255 > 0.7, encoder/heatmap.py:56-60, encoder/offset.py:46-50.
 * out: (N, round(h / stride), round(w / stride)) bytes 0 / 1.  Same published 8-bit algorithm as og_resize_cubic_u8
 * (pinned to oracle/og_oracle.c:ogo_shrink_mask_miss_u8; parity with cv2 itself unpinned). */
int og_shrink_mask_miss_u8(const unsigned char *mask, int N, int h, int w, int stride, unsigned char *out, void *stream);

/* The whole input chain of evaluate.py:150-168 in one pass: rescale to (new_h,new_w) as above, pad to (target_h,target_w)
 * with the fill colour -- corner_pad 0: CenterPad (transforms/pad.py:35-62, the --long-edge chain), 1: RightDownPad
 * (transforms/pad.py:70-118, the --fixed-height chain: left = top = 0) --, ToTensor, Normalize -> out fp32
 * (3,target_h,target_w); ltrb as og_center_pad_normalize_u8.  The resized uint8 image is never stored. */
int og_rescale_pad_normalize_u8(const unsigned char *img, int h, int w, int new_h, int new_w, int target_h, int target_w,
                                int corner_pad, const float *mean3, const float *std3, const float *fill3, float *out,
                                int *ltrb, void *stream);

/* The same chain for a whole batch in ONE launch (evaluate.py:157-182 collates the images of a batch before the network sees
 * them): `raw` = the batch's uint8 images packed back to back in HBM; offsets (host long[n]) = byte offset of image i;
 * hw4 (host int[4 n]) = (h, w, new_h, new_w) of image i; out fp32 (n,3,target_h,target_w); ltrb (host int[4 n] or NULL).
 * Bit-identical to n calls of og_rescale_pad_normalize_u8. */
int og_rescale_pad_normalize_batch_u8(const unsigned char *raw, const long *offsets, const int *hw4, int n, int target_h,
                                      int target_w, int corner_pad, const float *mean3, const float *std3, const float *fill3,
                                      float *out, int *ltrb, void *stream);

/* ---- network stem: convolution(7, 3, 128, stride=2) + BN + ReLU  models/hourglass_104.py:283, :16-30 ----
 * images (N,3,H,W) fp32 (H, W multiples of 32) -> out (N,H/2,W/2,128) bf16 NHWC, input conversion and epilogue fused.
 * w_packed bf16 [128][7 kernel rows][8 taps][4 channels] (tap 7 and channel 3 zero) = the BN-folded weight
 * (128,3,7,7) permuted to (cout, ky, kx, ch) and zero-padded; bias fp32[128]. */
int og_stem7x7_bf16(const float *images, const void *w_packed, const float *bias, void *out, int N, int H, int W, int relu,
                    void *stream);

/* ---- 3x3 stride-1 pad-1 convolution with the epilogue fused, for the small inner hourglass levels ----
 * out = act(conv3x3(x, w) + bias (+ skip)):  convolution.forward models/hourglass_104.py:26-30 / residual.forward
 * :70-79 with BN folded.  x (N,H,W,Cin), w (Cout,3,3,Cin) [= channels_last (Cout,Cin,3,3)], skip/out (N,H,W,Cout),
 * all bf16; bias fp32[Cout]; Cin, Cout multiples of 64; fp32 accumulation, one rounding to bf16.
 * Split-K implicit GEMM on MFMA: meant for N*H*W of a few hundred to a few thousand pixels, where library
 * kernels leave most CUs idle.  workspace: og_conv3x3_workspace_bytes(N*H*W, Cin, Cout), 256-byte aligned,
 * ZERO-INITIALISED once by the caller (its first 256 bytes are read as the zero padding and never written). */
int og_conv3x3_bf16(const void *x, const void *w, const float *bias, const void *skip, void *out, int N, int H, int W,
                    int Cin, int Cout, int relu, void *workspace, size_t workspace_bytes, void *stream);
size_t og_conv3x3_workspace_bytes(long pixels, int Cin, int Cout);        /* upper bound for any H x W with N*H*W = pixels */
size_t og_conv3x3_workspace_bytes_nhw(int N, int H, int W, int Cin, int Cout);  /* exact for this shape */
/* General form for the remaining convolutions of the hourglass: ksize 1 (pad 0) or 3 (pad 1), stride 1 or 2 --
 * residual.conv1 with stride 2 and the 1x1 projection `skip` (models/hourglass_104.py:54-57, :63-68), the 1x1
 * inters_/cnvs_ junction (:239-250) and the head convolutions (models/heads.py).  x (N,Hin,Win,Cin),
 * w (Cout,ksize,ksize,Cin), skip/out (N,Hout,Wout,Cout) with Hout = (Hin + 2*(ksize/2) - ksize)/stride + 1;
 * same dtype / channel / workspace rules as og_conv3x3_bf16 (which is og_conv2d_bf16 with ksize 3, stride 1);
 * workspace: og_conv2d_workspace_bytes (0 = unsupported shape). */
int og_conv2d_bf16(const void *x, const void *w, const float *bias, const void *skip, void *out, int N, int Hin, int Win,
                   int Cin, int Cout, int ksize, int stride, int relu, void *workspace, size_t workspace_bytes,
                   void *stream);
size_t og_conv2d_workspace_bytes(int N, int Hin, int Win, int Cin, int Cout, int ksize, int stride);
/* A whole projection residual tail in one launch: out = act(conv(x) + conv1x1(x2, stride2) + bias) -- residual.forward
 * models/hourglass_104.py:70-79 with the `skip` branch (:63-68) a 1x1 convolution + BN: bn2(conv2(.)) + skip(x), ReLU.
 * The projection is appended along K: w_cat (Cout, ksize*ksize*Cin + Cin2) = [conv weight (Cout,k,k,Cin) | projection
 * weight (Cout,Cin2)], x2 (N,H2,W2,Cin2) sampled at (y*stride2, x*stride2); bias = the sum of both folded biases.
 * Always the split-K kernel (meant for the small levels); workspace: og_conv2d_proj_workspace_bytes. */
int og_conv2d_proj_bf16(const void *x, const void *w_cat, const float *bias, const void *x2, void *out, int N, int Hin,
                        int Win, int Cin, int Cout, int ksize, int stride, int H2, int W2, int Cin2, int stride2, int relu,
                        void *workspace, size_t workspace_bytes, void *stream);
size_t og_conv2d_proj_workspace_bytes(int N, int Hin, int Win, int Cin, int Cout, int ksize, int stride, int Cin2);
/* ---- band-resident convolution for the SMALL levels (20x20 / 10x10 / 5x5 at batch 8): csrc/conv_band.hip.  A workgroup owns
 * (image, band of output rows, 16 output channels) and all of K; K is split over its four waves (wave w = a quarter of the input
 * channels, all nine taps), whose weight fragments go from the pre-packed image straight into registers; the band's input rows sit
 * in LDS once (zero pixels between the rows: a tap is a plain address shift); the waves' fp32 partial tiles meet in LDS: no slabs,
 * no tickets, nothing but finished activations is handed between workgroups.  Same arithmetic as og_conv2d_* / og_conv2d_proj_*
 * (fp32 accumulation over the same products, one rounding; the summation ORDER differs, so results agree to fp32 rounding, not bit
 * for bit).  Replaces convolution.forward models/hourglass_104.py:26-30 and residual.forward :70-79 (BN folded), stride 1 or 2,
 * with the residual's 1x1 projection `skip` (:63-68) as extra K steps.
 *   og_conv_band_supported: 0 = not served (needs 64 <= Cin (and Cin2) <= 512 in multiples of 32, Cout % 16 == 0, stride 1 | 2,
 *     pad 1, input width <= 112, a band's rows in 160 KiB of LDS); otherwise the number of workgroups of the launch.
 *   og_conv_band_pack_w16: w (Cout,3,3,Cin) = the memory of a channels_last (Cout,Cin,3,3) tensor [+ w2 (Cout,Cin2), or NULL with
 *     Cin2 = 0] -> packed, Cout * (9*Cin + Cin2) elements, once per layer.
 *   og_conv_band_*: x (N,Hin,Win,Cin), skip / out (N,H,W,Cout) with H = (Hin-1)/stride + 1, x2 (N,H2,W2,Cin2) sampled at
 *     (y*stride2, x*stride2) or NULL; bias fp32[Cout] (with a projection: the sum of both folded biases). */
int og_conv_band_supported(int N, int Hin, int Win, int Cin, int Cout, int stride, int H2, int W2, int Cin2, int stride2);
int og_conv_band_pack_w16(const void *w, const void *w2, int Cin, int Cout, int Cin2, void *packed, void *stream);
int og_conv_band_bf16(const void *x, const void *w_packed, const float *bias, const void *skip, const void *x2, void *out, int N,
                      int Hin, int Win, int Cin, int Cout, int stride, int relu, int H2, int W2, int Cin2, int stride2, void *stream);
int og_conv_band_f16(const void *x, const void *w_packed, const float *bias, const void *skip, const void *x2, void *out, int N,
                     int Hin, int Win, int Cin, int Cout, int stride, int relu, int H2, int W2, int Cin2, int stride2, void *stream);
/* ---- the same 3x3 stride-1 convolution for the LARGE levels (160x160 / 80x80 / 40x40 at 640x640 input), on weights tiled
 * once in advance: csrc/conv3x3_tiled.inc -- halo-tiled direct convolution, two 4-wave workgroups per CU, 32-channel K steps,
 * every weight stage one contiguous 8 KiB LDS image.  Same arithmetic and epilogue as og_conv3x3_bf16 (fp32 accumulation, the
 * residual initialises the accumulators, one rounding).
 *   og_conv3x3_tiled_supported: 0 = shape not served (needs Cout % 128 == 0, Cin % 64 == 0, and H, W multiples of 16, or
 *     W == 40 / W == 20 with H % 4 == 0), otherwise the tile kind (16 x 16, 40 x 4, 20 x 4 pixels).
 *   og_conv3x3_tiled_workspace_bytes: 0 for most shapes (workspace may then be NULL).  A level whose output tiles alone would
 *     not fill the chip (40 x 40 and 20 x 20 at batch 8) is also split along K over 2-3 workgroups per tile, which meet through
 *     fp32 slabs + arrival tickets in the workspace: 256-byte aligned, ZERO-INITIALISED once by the caller, reusable by any
 *     later call on the same stream.
 *   og_conv3x3_pack_w16: w (Cout,3,3,Cin) 16-bit (bf16 or fp16 alike) -> packed, the same number of bytes, laid out
 *     [Cout/128][Cin/32][9 taps][128 rows x 64 B] with the k order / slot swizzle the kernel's fragment reads expect;
 *     order 0 = taps in their own order (for og_conv3x3_tiled_*), order 1 = the order the stride-2 kernel consumes them
 *     (0 2 6 8 | 3 5 | 1 7 | 4, for og_conv3x3s2_tiled_*); order 2 / 3 = a 1x1 weight (Cout, Cin) in cout tiles of 128 / 64 rows
 *     with k in its natural order (for og_conv1x1_tiled_* / og_conv1x1_heads_*).
 *   og_conv3x3_tiled_bf16: x (N,H,W,Cin), skip / out (N,H,W,Cout), bias fp32[Cout]; replaces convolution.forward
 *     models/hourglass_104.py:26-30 / residual.forward :70-79 (BN folded) like og_conv3x3_bf16. */
/* Optional hint for the NEXT convolution launch issued by this host thread -- og_conv3x3_tiled_* / og_conv3x3_tiled_up2_* /
 * og_conv3x3s2_tiled_* / og_conv_band_* / og_conv2d_* / og_conv2d_proj_* / og_conv3x3_* (every launch of the five takes and clears it;
 * the 1x1 kernels og_conv1x1_* and the stem do not look at it): [w_next, w_next + bytes) = the packed weights of the layer that will run AFTER that launch.  The launch's
 * workgroups touch those lines at entry (values unused), so that the next layer of a dependent chain -- the 20x20 / 10x10 / 5x5 levels,
 * whose layers are bound by the latency of first-touch weight reads -- finds its weights in the memory-side cache instead of HBM.
 * Purely a performance hint: results do not depend on it; NULL / 0 clears it. */
void og_conv_next_weights_hint(const void *w_next, size_t bytes);
int og_conv3x3_tiled_supported(int N, int H, int W, int Cin, int Cout);
int og_conv3x3_pack_w16(const void *w, int Cin, int Cout, int order, void *packed, void *stream);
size_t og_conv3x3_tiled_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int og_conv3x3_tiled_bf16(const void *x, const void *w_packed, const float *bias, const void *skip, void *out, int N, int H,
                          int W, int Cin, int Cout, int relu, void *workspace, size_t workspace_bytes, void *stream);
/* The last convolution below an hourglass merge and the merge itself in one launch (kp_module.forward, models/hourglass_104.py:
 * 170-176: up2 = upsample(low3); return up1 + up2): up (N,2H,2W,Cout), holding up1, += nearest_x2(act(conv3x3(x) + bias + skip)),
 * the convolution's result rounded to 16 bits first -- og_conv3x3_tiled_bf16 followed by og_upsample2_add_bf16, bit for bit; the
 * (N,H,W,Cout) tensor in between is never written.  Shapes and workspace as og_conv3x3_tiled_bf16. */
int og_conv3x3_tiled_up2_bf16(const void *x, const void *w_packed, const float *bias, const void *skip, void *up, int N, int H,
                              int W, int Cin, int Cout, int relu, void *workspace, size_t workspace_bytes, void *stream);
/* Stride 2 (residual.conv1 of the down-sampling residuals, models/hourglass_104.py:54-57 with stride 2, and the second `pre`
 * layer :214-217) on the same kernel structure: x (N,Hin,Win,Cin) -> out (N,Hin/2,Win/2,Cout), pad 1; weights packed with
 * order 1; the four input-parity phases of a tile are gathered straight from the NHWC input by the LDS-DMA.
 * og_conv3x3s2_tiled_supported(N, Hin, Win, Cin, Cout): 0 = not served; needs Hin, Win even, Cout % 128 == 0, Cin % 64 == 0 and
 * an output of 8k x 16k pixels (1: 16 x 8 output tiles) or 40 wide with an even height (2: 40 x 2 tiles, the 80 -> 40 level). */
int og_conv3x3s2_tiled_supported(int N, int Hin, int Win, int Cin, int Cout);
int og_conv3x3s2_tiled_bf16(const void *x, const void *w_packed, const float *bias, const void *skip, void *out, int N, int Hin,
                            int Win, int Cin, int Cout, int relu, void *stream);
/* ---- pointwise (1x1) convolutions of the large levels (csrc/conv3x3_tiled.inc, conv1x1_tiled_kernel) ----
 * og_conv1x1_tiled_bf16: out (N,H,W,Cout) = act(W [x1 | x2] + bias (+ skip)): output pixel (y, x) reads x1 (N,H1,W1,C1) at
 *   (y * stride1, x * stride1); an optional second input x2 of the SAME shape and stride is concatenated along K -- the
 *   inters_ / cnvs_ junction relu(bn(conv(inter)) + bn(conv(feat))) of models/hourglass_104.py:239-250, :291-292 in one launch --
 *   and stride 2 with one input is the 1x1 projection `skip` of the down-sampling residuals (:63-67).  w_packed: the
 *   (Cout, C1 + C2) weight through og_conv3x3_pack_w16(order 2); C1, C2 multiples of 64, Cout of 128; bias / skip may be null.
 * og_conv1x1_heads_bf16: all heads of the decoded stack as one 1x1 convolution (models/heads.py:48-70, :116-142, no
 *   activation): x (N,H,W,C) -> up to four dense fp32 NCHW tensors outs[i] (N,head_channels[i],H,W), written straight from the
 *   fp32 accumulators (bias added in fp32, no 16-bit rounding).  w_packed: the concatenated head weights padded to Cout (a
 *   multiple of 64) through og_conv3x3_pack_w16(order 3); bias fp32[Cout]. */
int og_conv1x1_tiled_bf16(const void *x1, int C1, int H1, int W1, int stride1, const void *x2, int C2, int H2, int W2, int stride2,
                          const void *w_packed, const float *bias, const void *skip, void *out, int N, int H, int W, int Cout,
                          int relu, void *stream);
int og_conv1x1_heads_bf16(const void *x, int C, const void *w_packed, const float *bias, int N, int H, int W, int Cout, int n_heads,
                          const int *head_channels, float *const *outs, void *stream);
/* Debug aid: later og_conv3x3_bf16 launches write [workgroup][8] u64 s_memrealtime (100 MHz) marks into `buf`
 * (device memory, 64 B per workgroup); NULL switches it off. */
/* ---- the same entry points for fp16 activations / weights (the reference evaluates in fp16 through apex O2,
 * evaluate.py:92,198-201): v_mfma_f32_16x16x32_f16 instead of ..._bf16, fp32 accumulation, identical layouts, arguments,
 * workspaces (og_conv*_workspace_bytes) and error behaviour; models.InferenceEngine(dtype=torch.float16).
 * At the ends of the fp16 range -- observed on gfx950 on the 29 small shapes of tests/test_gpu_conv_exact.py (*_range) and the directed
 * cases of tests/test_gpu_range_glue.py, an observation those tests hold, not a guarantee beyond them: subnormal fp16 weights and
 * activations went through the MFMA, the stem's input conversion, the phase images, skip / up operands and the weight packers
 * unflushed; outputs below 2^-14 were rounded to nearest even on the subnormal grid; outputs that round beyond 65504 came out as
 * +-inf, not clamped; og_conv1x1_heads_f16 wrote the fp32 value unrounded. ---- */
int og_bias_act_f16(void *x, const float *bias, const void *skip, long pixels, int channels, int relu, void *stream);
int og_upsample2_add_f16(void *up, const void *low, long n, int H, int W, int channels, void *stream);
int og_nchw_f32_to_nhwc_f16(const float *src, void *dst, long N, int C, int H, int W, void *stream);
int og_nhwc_f16_to_nchw_f32(const void *src, int src_channels, int first_channel, int channels, const float *bias,
                            float *dst, long N, int H, int W, void *stream);
int og_stem7x7_f16(const float *images, const void *w_packed, const float *bias, void *out, int N, int H, int W, int relu,
                   void *stream);
int og_conv3x3_f16(const void *x, const void *w, const float *bias, const void *skip, void *out, int N, int H, int W,
                   int Cin, int Cout, int relu, void *workspace, size_t workspace_bytes, void *stream);
int og_conv3x3_tiled_f16(const void *x, const void *w_packed, const float *bias, const void *skip, void *out, int N, int H,
                         int W, int Cin, int Cout, int relu, void *workspace, size_t workspace_bytes, void *stream);
int og_conv3x3_tiled_up2_f16(const void *x, const void *w_packed, const float *bias, const void *skip, void *up, int N, int H,
                         int W, int Cin, int Cout, int relu, void *workspace, size_t workspace_bytes, void *stream);
int og_conv3x3s2_tiled_f16(const void *x, const void *w_packed, const float *bias, const void *skip, void *out, int N, int Hin,
                           int Win, int Cin, int Cout, int relu, void *stream);
int og_conv1x1_tiled_f16(const void *x1, int C1, int H1, int W1, int stride1, const void *x2, int C2, int H2, int W2, int stride2,
                         const void *w_packed, const float *bias, const void *skip, void *out, int N, int H, int W, int Cout,
                         int relu, void *stream);
int og_conv1x1_heads_f16(const void *x, int C, const void *w_packed, const float *bias, int N, int H, int W, int Cout, int n_heads,
                         const int *head_channels, float *const *outs, void *stream);
int og_conv2d_f16(const void *x, const void *w, const float *bias, const void *skip, void *out, int N, int Hin, int Win,
                  int Cin, int Cout, int ksize, int stride, int relu, void *workspace, size_t workspace_bytes, void *stream);
int og_conv2d_proj_f16(const void *x, const void *w_cat, const float *bias, const void *x2, void *out, int N, int Hin,
                       int Win, int Cin, int Cout, int ksize, int stride, int H2, int W2, int Cin2, int stride2, int relu,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ---- training losses, value + gradient in one pass ----
 * og_focal_l2_loss_f32: models/losses.py:31-58 + HeatMapsLoss :174-176.  pred/gt (N,C,hw) fp32, mask_miss
 *   (N,hw) bytes (0 = unlabelled); *sum += sum of 0.5 (s-s*)^2 |1-st|^gamma over labelled elements with finite
 *   gt (caller zeroes *sum); grad (N,C,hw) = d sum / d pred.
 * og_offset_l1_loss_f32: offset_instance_l1_loss :87-92 + OffsetMapsLoss :237-242.  e = |pred/ps - gt/ps| kept
 *   if e >= margin (sqrt(e) if sqrt_re); sum_count[0] += sum, sum_count[1] += count; grad = d sum / d pred
 *   (the caller scales by 1 / (1 + count)).
 * All six loss entry points ADD to *sum / sum_count[0..1] with float atomics (one per wave) and never overwrite them: what the
 *   caller left there stays in the result, and the count is a float. */
int og_focal_l2_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw,
                         float tau, float gamma, float *sum, float *grad, void *stream);
int og_offset_l1_loss_f32(const float *pred, const float *gt, const float *gt_ps, const unsigned char *mask_miss, int N,
                          int C, long hw, float margin, int sqrt_re, float *sum_count, float *grad, void *stream);
/* The remaining loss choices and the optional heads (LossChoice :61-137), same conventions: caller-zeroed accumulators,
 * gradient of the SUM written in the same pass, 0 for every dropped element (unlabelled, non-finite target, below margin).
 * 16-byte accesses when hw % 4 == 0 and the pointers are 16-byte aligned, else 4-byte.
 * og_l2_loss_f32: *sum += sum of 0.5 (p-g)^2 over labelled elements with finite gt; grad = p-g.
 * og_masked_l1_loss_f32: e = |p-g| over labelled elements with finite gt (keypoint scales: NaN outside the patches; jitter
 *   offsets: inf), kept if e >= margin (sqrt(e) if sqrt_re); sum_count[0] += sum, sum_count[1] += count.
 * og_vector_l1_loss_f32: channels (2l, 2l+1) of pred/gt (N,C,hw), C even, are one vector: r = sqrt(dx^2 + dy^2), kept where
 *   labelled, r finite and r >= margin (sqrt(r) if sqrt_re); grad = d/r per component (x 0.5/sqrt(r)).
 * og_laplace_loss_f32: r as above, v = logb + r exp(-logb) with logb (N,C/2,hw) (the spread head), kept where labelled, r
 *   finite and v >= margin (sqrt(v) if sqrt_re); grad (N,C,hw) = d sum / d pred, grad_logb (N,C/2,hw) = d sum / d logb. */
int og_l2_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw, float *sum,
                   float *grad, void *stream);
int og_masked_l1_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw,
                          float margin, int sqrt_re, float *sum_count, float *grad, void *stream);
int og_vector_l1_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw,
                          float margin, int sqrt_re, float *sum_count, float *grad, void *stream);
int og_laplace_loss_f32(const float *pred, const float *gt, const float *logb, const unsigned char *mask_miss, int N, int C,
                        long hw, float margin, int sqrt_re, float *sum_count, float *grad, float *grad_logb, void *stream);

/* ---- ground-truth encoder ----
 * joints (N,P,n_kp,4) fp32 rows [x, y, v, scale] in input-image pixels (transforms/annotations.py:46-50), P = padded
 * person count, n_persons int32[N] (NULL: all P rows are used; rows with v <= 0 never contribute).
 * og_encode_heatmaps_f32: HeatMapGenerator.create_heatmaps encoder/heatmap.py:125-197 -> hm (N,n_kp,h,w) and, if not
 *   NULL, bg (N,1,h,w) = 1 - max over channels (:78); h = in_h/stride, w = in_w/stride.
 * og_encode_offsets_f32: OffsetMapGenerator.create_offsetmaps encoder/offset.py:98-197 -> off (N,2L,h,w) (inf where no
 *   limb is defined), pscale (N,2L,h,w) (1 there), and, if not NULL, scale (N,n_kp,h,w) (nan there); jf/jt int32[L],
 *   sigmas fp32[n_kp] (config COCO_PERSON_SIGMAS) are device arrays.
 * Offsets/scales bit-exact vs the reference; heatmaps to ~2e-7 (device exp). */
int og_encode_heatmaps_f32(const float *joints, const int32_t *n_persons, int N, int P, int n_kp, int in_w, int in_h,
                           int stride, int sigma, float clip_thre, float *hm, float *bg, void *stream);
/* og_encode_jitter_f32: HeatMapGenerator.create_jitter_offset encoder/heatmap.py:199-255 -> jit (N,2,h,w): vector from
 * the cell centre to the nearest annotated keypoint inside a fill_size window, inf elsewhere (bit-exact). */
int og_encode_jitter_f32(const float *joints, const int32_t *n_persons, int N, int P, int n_kp, int in_w, int in_h,
                         int stride, int fill_size, float *jit, void *stream);
int og_encode_offsets_f32(const float *joints, const int32_t *n_persons, int N, int P, int n_kp, const int32_t *jf,
                          const int32_t *jt, int L, int in_w, int in_h, int stride, int fill_size, float min_jscale,
                          const float *sigmas, float *off, float *scale, float *pscale, void *stream);

/* ---- pose painter (visualization/__init__.py:draw_poses, evaluate.py --show-detected-poses) ----
 * Paints skeletons over images (N,H,W,3) uint8 RGB IN PLACE: what the reference's KeypointPainter.keypoints shows
 * (visualization/show.py:225-253 -- one colour per person, limbs with round caps, a marker per visible keypoint, no box) as a
 * capsule / disc rasteriser of this library's own, not matplotlib's renderer.  All pointers are device pointers:
 * poses (N,P,K,3) fp32 rows x, y, v in pixel coordinates of `images`; n_persons int32[N], persons in use per image (clamped
 * to [0, P]; the rows beyond are never read); skeleton int32 (L,2), ZERO-based keypoint indices (a limb with an index outside
 * [0, K) is skipped); palette (n_colors,3) uint8.  No workspace.
 * Primitives of image n, in this order: for person p = 0 .. n_persons[n]-1 the L limbs in skeleton order, then the K
 * keypoints in index order.  A limb (a, b) is a capsule of radius r = line_width / 2 between the two keypoints, drawn only if
 * both have v > 0 and all four coordinates are finite; a keypoint is a disc of radius r = marker_radius, drawn only if v > 0
 * and its coordinates are finite.  Colour: palette[p % n_colors].  The centre of the pixel in column i, row j is (i, j).
 * Coverage of a pixel centre (px, py): cov = clamp(r + 0.5 - d, 0, 1), d its distance to the segment / the disc centre, with
 *   dx = bx - ax, dy = by - ay, len2 = dx*dx + dy*dy,
 *   t = clamp(((px - ax)*dx + (py - ay)*dy) / len2, 0, 1), t = 0 when len2 == 0 (and for a disc),
 *   qx = ax + t*dx, qy = ay + t*dy, d = sqrt((px - qx)*(px - qx) + (py - qy)*(py - qy)),
 * every operation one IEEE fp32 operation, left to right as written, no contraction, correctly rounded divide and square
 * root; clamp(x, 0, 1) = fmin(fmax(x, 0), 1).  A pixel keeps its three channels in fp32 and, for every primitive with cov > 0
 * in primitive order, c = c + (colour - c) * (cov * alpha); a pixel no primitive covers is never written, a covered one is
 * stored once as (uint8) floor(c + 0.5).  Blending does not commute: the order is part of the result.
 * OG_EINVAL (nothing launched): a null pointer, a non-positive N, H, W, P, K or L, n_colors <= 0, alpha outside (0, 1], a
 * negative or non-finite line_width / marker_radius, N or ceil(H / 8) beyond 65535. */
int og_draw_poses_u8(void *images, const float *poses, const int *n_persons, const int *skeleton,
                     const unsigned char *palette, int n_colors, int N, int H, int W, int P, int K, int L,
                     float line_width, float marker_radius, float alpha, void *stream);

/* ---- model-inspection views (visualization/__init__.py: draw_heatmap, draw_segments, draw_limbs, draw_offsets; evaluate.py
 * --show-hmp-idx / --show-all-limbs / --show-limb-idx: the views of the reference's demo_batch.py:215-317) ----
 * Rasterisers of this library's own over images uint8 RGB IN PLACE, and the two compactions that feed the segment painter.  All
 * pointers are device pointers, no call needs a workspace, everything is ordered on `stream` and may be captured.  In all of them
 * every operation written below is one IEEE fp32 operation, left to right as written, no contraction, divides correctly rounded.
 *
 * og_draw_heatmap_u8: one heat-map channel over images (N,4h,4w,3).  hm (N,C,h,w) fp32 is the stride-4 head output, lut
 * (n_colors,3) uint8 the colour table.  For the pixel in row Y, column X of image n:
 *   v = the element (n, channel, Y, X) og_upsample_bicubic4_f32 writes for hm (the x4 plane itself is never built);
 *   nms == 0: u = v;  nms != 0: m = the largest of the nine v of the 3 x 3 window round (Y, X), a neighbour outside the image
 *   counting as 0 and a NaN never as the larger one, and u = v * (m == v ? 1.f : 0.f) -- og_hmp_nms_f32's result on the x4 plane;
 *   a NaN u leaves the pixel unwritten; otherwise t = fmin(fmax((u - vmin) / (vmax - vmin), 0), 1),
 *   idx = (int) floorf(t * (float)(n_colors - 1) + 0.5f), and each channel c = (float) pixel; c = c + ((float) lut[idx][ch] - c) * alpha
 *   is stored as (uint8) floorf(c + 0.5f).
 * OG_EINVAL (nothing launched): a null pointer; a non-positive N, C, h or w, or h or w beyond INT_MAX / 4; channel outside [0, C);
 * n_colors <= 0; vmin or vmax not finite, or vmax <= vmin; alpha outside (0, 1]; N or ceil(4h / 16) beyond 65535. */
int og_draw_heatmap_u8(void *images, const float *hm, const unsigned char *lut, int n_colors, int N, int C, int h, int w,
                       int channel, float vmin, float vmax, float alpha, int nms, void *stream);

/* og_draw_segments_u8: line segments with end markers over images (N,H,W,3).  segs (N,S,4) fp32 rows x1, y1, x2, y2 in pixel
 * coordinates of `images`, 16-byte aligned; n_segs int32[N], rows in use per image (clamped to [0, S]; the rows beyond are never
 * read); line_rgb / marker_rgb: one colour each, passed by value as r | g << 8 | b << 16 (higher bits ignored).
 * Primitives of image n, in this order: for s = 0 .. n_segs[n]-1 a capsule of radius line_width / 2 from (x1, y1) to (x2, y2) in
 * line_rgb, then, if r_start > 0, a disc of radius r_start at (x1, y1) in marker_rgb, then, if r_end > 0, a disc of radius r_end at
 * (x2, y2) in marker_rgb.  A segment with a non-finite coordinate is skipped whole, discs included.  Coverage, blending in
 * primitive order, rounding and the rule that a pixel no primitive covers is never written are those of og_draw_poses_u8 above.
 * OG_EINVAL (nothing launched): a null pointer; a non-positive N, H, W or S; alpha outside (0, 1]; a negative or non-finite
 * line_width, r_start or r_end; segs not 16-byte aligned; 3 S beyond 2^30; N or ceil(H / 8) beyond 65535. */
int og_draw_segments_u8(void *images, const float *segs, const int *n_segs, int N, int H, int W, int S, unsigned int line_rgb,
                        unsigned int marker_rgb, float line_width, float r_start, float r_end, float alpha, void *stream);

/* og_limbs_to_segments_f32: the candidate limbs the pairing produced as segment rows (demo_batch.py:267-276).  limbs (N,L,K,13)
 * fp32 is the output of the og_generate_limbs_* / og_collect_limbs_* calls (columns x1, y1, v1, x2, y2, v2, ind1, ind2, len_delta,
 * ...).  Row (l, i) of image n is kept iff (limb < 0 || l == limb) && col0 > 0 && col3 > 0 && col8 <= dist_max (a comparison with
 * a NaN is false); a kept row gives the segment [col0, col1, col3, col4].  The kept rows of image n are written to
 * segs (N,L*K,4) from row 0 on in ascending (l, i) order, their number to n_segs[n]; rows of segs past it are left untouched.
 * OG_EINVAL (nothing launched): a null pointer; a non-positive N, L or K, or L * K beyond 2^28; limb >= L; segs not 16-byte aligned. */
int og_limbs_to_segments_f32(const float *limbs, int N, int L, int K, int limb, float dist_max, float *segs, int *n_segs,
                             void *stream);

/* og_offsets_to_segments_f32: the guiding offsets of one limb type as arrows (visualization/show.py:52-64).  hm (N,C,h,w) and off
 * (N,2L,h,w) fp32 are the stride-4 head outputs.  Grid points (Y, X), Y = 0, step, 2 step, ... < 4h and X likewise < 4w, in
 * row-major order: S = og_offsets_segments_capacity(h, w, step) = ceil(4h / step) * ceil(4w / step) of them (0 for a non-positive
 * argument: host arithmetic).  At a point, heat = the element og_upsample_bicubic4_f32 writes for channel joint_from of hm, U and V
 * the elements og_upsample_bilinear4_f32 writes for channels 2 limb and 2 limb + 1 of off (bilinear: the decoder's own resampling
 * of the offsets).  The point is kept iff heat >= thre and U and V are finite (the reference masks heat < thre and sets infinite
 * offsets to zero: here such an arrow is dropped); a kept point gives [(float) X, (float) Y, (float) X + U, (float) Y + V].  Output
 * as above: segs (N,S,4) in grid order from row 0 on, n_segs[n], the rest untouched.
 * OG_EINVAL (nothing launched): a null pointer; a non-positive N, C, L, h or w, or h or w beyond 2^22; joint_from outside [0, C);
 * limb outside [0, L); step <= 0; segs not 16-byte aligned; S beyond 2^28. */
long og_offsets_segments_capacity(int h, int w, int step);
int og_offsets_to_segments_f32(const float *hm, const float *off, int N, int C, int L, int h, int w, int joint_from, int limb,
                               int step, float thre, float *segs, int *n_segs, void *stream);

/* ---- training augmentation (transforms/affine.py:71-278, WarpAffineTransforms; offsetguided_amd.transforms.DeviceAugment) ----
 * og_warp_affine_batch_u8: warp + ToTensor + Normalize of a batch in ONE launch.  `raw`, `offsets` (host long[n]) and `hw4` (host
 * int[4 n]; entries (h, w, -, -) of image i, the last two unused here) as og_rescale_pad_normalize_batch_u8 takes them; D (host
 * double[6 n]) = the first two rows of inv(M) of image i, row-major [a b c; d e f]: destination pixel (x, y) of the S x S square reads
 * the source round (a x + b y + c, d x + e y + f); border3 (host, 3 bytes; the reference fills 124, 116, 104), mean3 / std3 (host, 3
 * floats).  out fp32 (n,3,S,S) = (v / 255 - mean) / std with v the warped 8-bit value; out_u8 (device, (n,S,S,3), may be NULL)
 * receives v itself.  The warp is this library's own integer specification -- 32 sub-pixel phases, 4-tap cubic (A = -0.75) taps
 * scaled to 2^11 that sum to 2048, (sum + 2^21) >> 22, taps outside the image read the border colour -- written out operation by
 * operation in csrc/augment.hip and held bit for bit to the numpy restatement tests/augment_common.py; bit parity with
 * cv2.warpAffine(INTER_CUBIC) is NOT claimed (third-party, absent from the build).
 * og_warp_affine_mask_u8: the same warp of single-channel planes (mask_miss, border 255 in the reference) -> out (n,S,S) uint8.
 * OG_EINVAL (nothing launched): a null pointer; a non-positive n, S, h or w, S beyond 16384, h w beyond 2^28; a D that is not finite
 * or with |a| S + |b| S + |c| >= 2^20 (likewise d, e, f): the kernel works in int32.
 * og_affine_joints_f32: _affine_keypoints (:192-227) for joints (N,P,K,4) fp32 rows [x, y, v, scale] (device, 16-byte aligned),
 * n_persons int32[N] (device; NULL: all P rows): M (host double[6 N]) the first two rows of the forward matrix, flip (host int[N]),
 * scale (host double[N]) = sqrt(scale_x scale_y), left / right (host int[n_lr], n_lr <= 16) the mirror partners.  Per row of a
 * person in use: x' = (m0 x + m1 y) + m2 in float64, products rounded before the sums, left to right, stored as fp32; y' with the
 * second row; column 3 times scale in float64, rounded to fp32; with flip the rows of left[i] and right[i] change places; then
 * v = 0 where x' <= 0 or y' <= 0 or x' > S_w or y' > S_h (on the fp32 values).  Rows beyond n_persons[n] are copied unchanged. */
int og_warp_affine_batch_u8(const unsigned char *raw, const long *offsets, const int *hw4, int n, const double *D, int S,
                            const unsigned char *border3, const float *mean3, const float *std3, float *out, unsigned char *out_u8,
                            void *stream);
int og_warp_affine_mask_u8(const unsigned char *masks, const long *offsets, const int *hw4, int n, const double *D, int S, int border,
                           unsigned char *out, void *stream);
int og_affine_joints_f32(const float *joints, const int *n_persons, int N, int P, int K, const double *M, const int *flip,
                         const double *scale, float S_w, float S_h, const int *left, const int *right, int n_lr, float *out,
                         void *stream);

/* ---- photometric training augmentation (transforms/image.py:31-41, 55-86; transforms/annotations.py:89-111; DeviceAugment with
 * PhotoParams) ----  The per-image photometric table photo4 (host int[4 n]) holds {mode, dh, ds, dv}: mode bit 0 = ColorTint with
 * the deltas (dh, ds, dv) added to H in [0, 180) (clamped to [0, 179], not wrapped), S and V in [0, 255]; bit 1 = Gray
 * ((19595 R + 38470 G + 7471 B + 2^15) >> 16 on all three channels, PIL's `L`); tint first.  Both are integer specifications of this
 * library's own, written out in csrc/photometric.h and held bit for bit to tests/photometric_common.py; the tint has the shape of
 * OpenCV's 8-bit HSV conversion, parity with cv2.cvtColor is NOT claimed (absent from the build); Gray is pinned to PIL.
 * og_warp_affine_photo_batch_u8: og_warp_affine_batch_u8 with that epilogue between the warped value v and the normalisation: out
 * = normalise(epilogue(v)); out_u8 (may be NULL) still receives v itself.  With every mode 0 the output equals the plain entry's.
 * OG_EINVAL as the plain entry, and for a mode beyond 3, |dh| > 180, |ds| > 255 or |dv| > 255.
 * og_jpeg_roundtrip_batch_u8: JpegCompression.  u8 (device, (N,S,S,3)) = the out_u8 of the warp; for each of the n_selected image
 * indices in `selected` (host int[]) the planes of out (N,3,S,S) fp32 are overwritten with normalise(epilogue(jpeg(v))), the other
 * images' planes are not touched; photo4 (host int[4 N], indexed by image; NULL: no epilogue).  jpeg = the shape of baseline JPEG at
 * 4:2:0 in integer arithmetic of this library's own (16-bit fixed-point YCbCr, 2 x 2 chroma mean, 8 x 8 DCT as two integer matrix
 * products, Annex K tables scaled by `quality` the libjpeg way, box chroma upsampling, partial MCUs padded by replication),
 * csrc/jpeg_sim.hip; no bit parity with libjpeg, closeness to PIL measured (profiles/photometric_parity.json).
 * OG_EINVAL (nothing launched): a null pointer; non-positive N or S, S beyond 16384, negative n_selected; quality outside [1, 100];
 * a selected index outside [0, N); a bad descriptor of a selected image.  n_selected == 0 launches nothing.
 * og_affine_joints_jitter_f32: og_affine_joints_f32, then AnnotationJitter on the rows of persons in use of the images with gate[n]
 * != 0 (host int[N]): x' += eps[n] * (((u_x - 0.5) + shift[n]) * 2), y' likewise, every operation one fp32 operation in this order;
 * noise (device, (N,P,K,2) fp32, 8-byte aligned) holds u of OUTPUT row (n, p, k); eps, shift host float[N].  v is not re-tested (the
 * reference jitters after the warp).  An image with gate 0, and every padding row, equals og_affine_joints_f32. */
int og_warp_affine_photo_batch_u8(const unsigned char *raw, const long *offsets, const int *hw4, int n, const double *D, int S,
                                  const unsigned char *border3, const float *mean3, const float *std3, float *out,
                                  unsigned char *out_u8, const int *photo4, void *stream);
int og_jpeg_roundtrip_batch_u8(const unsigned char *u8, int N, int S, const int *selected, int n_selected, int quality,
                               const int *photo4, const float *mean3, const float *std3, float *out, void *stream);
int og_affine_joints_jitter_f32(const float *joints, const int *n_persons, int N, int P, int K, const double *M, const int *flip,
                                const double *scale, float S_w, float S_h, const int *left, const int *right, int n_lr,
                                const float *noise, const int *gate, const float *eps, const float *shift, float *out, void *stream);

/* ---- COCO keypoint scoring (COCOeval with iouType='keypoints', pycocotools/cocoeval.py: computeOks, evaluateImg;
 * offsetguided_amd.cocoeval.KeypointEval) ----  Packed batches of I images, all arithmetic IEEE double.  Image i owns detections
 * det_off[i] .. det_off[i + 1] (already sorted by descending score and truncated, at most 64 each), ground truths gt_off[i] ..
 * gt_off[i + 1] (file order, any count) and the row-major d_i x g_i block of `oks` that starts at pair_off[i] (the running sum of d_i
 * g_i).  det_off, gt_off (int32[I + 1]) and pair_off (int64[I + 1]) are device pointers; D, G and n_pairs are their last entries.
 * og_oks_matrix_f64: dets (D,17,3) and gts (G,17,3) rows [x, y, v], gt_area[G], gt_bbox[4 G] rows [x, y, w, h], sigmas (host
 * double[17]) -> oks[n_pairs].  One thread per pair, the image found by bisection over pair_off.  var[k] = (2 sigmas[k])^2; k1 = the
 * number of keypoints with vg > 0.  k1 > 0: dx = xd - xg, dy = yd - yg, only the keypoints with vg > 0 enter.  k1 == 0: every
 * keypoint enters with x0 = bx - bw, x1 = bx + 2 bw, y0 = by - bh, y1 = by + 2 bh, dx = max(0, x0 - xd) + max(0, xd - x1), dy
 * likewise.  e = (dx dx + dy dy) / var[k] / (area_g + 2^-52) / 2, evaluated left to right, no contraction; OKS = the sum of exp(-e)
 * in ascending k (the device's double exp) divided by the number of keypoints that enter.  n_pairs == 0 launches nothing.
 * og_oks_match_i32: the greedy matching of every (image, area range a, threshold t) in one launch -- one wavefront per image, lane
 * a T + t.  area_ranges (host double[2 A]) rows [lo, hi], thresholds (host double[T]); gt_ignore / gt_crowd uint8[G], det_area[D].
 * gt_ignore_a[a, g] = gt_ignore[g] || area_g < lo_a || area_g > hi_a.  Per detection in order: best = min(t, 1 - 1e-10), m = none;
 * the ground truths are visited with gt_ignore_a == 0 first, then the others, each group in file order; one that is matched already at
 * this (a, t) and is not crowd is skipped; the walk stops at the first ignored one once m is set and not ignored; OKS < best is
 * skipped; otherwise best = OKS, m = g (an equal OKS replaces).  m set: dt_match = m + 1 (m counted within the image), dt_ignore =
 * gt_ignore_a[a, m], g is marked; else dt_match = 0 and dt_ignore = det_area < lo_a || det_area > hi_a.  Outputs dt_match int32
 * (A,T,D), dt_ignore uint8 (A,T,D), gt_ignore_a uint8 (A,G).  The matched set of a lane is a bit mask for g_i <= 64 and a slice of
 * `workspace` above (og_oks_match_workspace_bytes(G, A, T), host arithmetic; always required); the image's OKS block is staged in LDS
 * up to 1024 pairs and read from global memory above.  Both kernels: no allocation, no synchronisation, graph-capturable.
 * OG_EINVAL (nothing launched): a null pointer; I <= 0; negative D, G or n_pairs; A or T outside 1..16 or A T > 64; a non-positive
 * sigma; and, where an offset table is host-visible (pinned), a table that decreases, does not run from 0 to its total, a pair_off
 * step that is not d_i g_i, or a d_i > 64 (a device-only table is not read by the host: the kernels then treat an image whose entries
 * leave the totals as empty).  OG_ENOSPC: workspace_bytes too small. */
int og_oks_matrix_f64(const double *dets, const double *gts, const double *gt_area, const double *gt_bbox, const int32_t *det_off,
                      const int32_t *gt_off, const int64_t *pair_off, const double *sigmas, int I, int D, int G, int64_t n_pairs,
                      double *oks, void *stream);
size_t og_oks_match_workspace_bytes(int G, int A, int T);
int og_oks_match_i32(const double *oks, const int32_t *det_off, const int32_t *gt_off, const int64_t *pair_off, const double *gt_area,
                     const unsigned char *gt_ignore, const unsigned char *gt_crowd, const double *det_area, const double *area_ranges,
                     int A, const double *thresholds, int T, int I, int D, int G, int64_t n_pairs, int32_t *dt_match,
                     unsigned char *dt_ignore, unsigned char *gt_ignore_a, void *workspace, size_t workspace_bytes, void *stream);

/* ---- mask_miss / mask_all from COCO annotations (data/dataset.py:136-197, CocoKeypoints.mask_mask, which calls pycocotools'
 * annToMask; offsetguided_amd.data.device_masks) ----  One call builds both masks of a batch of images of different sizes on the
 * device from the person annotations' polygons and run-length encodings.  The rule below has the shape of pycocotools' maskApi
 * (rleFrPoly, rleDecode); bit parity with pycocotools is NOT claimed (absent from the build): what is pinned is this text and its
 * numpy restatement tests/coco_mask_common.py, which is written in the sort-and-merge run-length form.
 * A mask plane of an h x w image is the flat COLUMN-MAJOR bit string a = x h + y, 0 <= a < h w.  Every source contributes toggle
 * positions; bit a of the plane is the XOR of the toggles at positions <= a.  The parity runs across column ends: a toggle at y = h
 * of column x is position (x + 1) h; a toggle at h w has no effect.
 * Polygon of k >= 1 vertices (px_j, py_j), float64.  All arithmetic IEEE double, every product rounded before the sum (no
 * contraction), (int) truncates toward zero:
 *   1. X_j = (int)(5 px_j + .5), Y_j = (int)(5 py_j + .5); vertex k is vertex 0.
 *   2. Edge (xs, ys) -> (xe, ye), j = 0 .. k - 1: dx = |xe - xs|, dy = |ys - ye|; flip = (dx >= dy and xs > xe) or (dx < dy and
 *      ys > ye); a flipped edge swaps its ends.  dx >= dy: s = (double)(ye - ys) / dx, the edge emits the dx + 1 points (u, v) =
 *      (xs + t, (int)(ys + s t + .5)) with t running 0 .. dx, or dx .. 0 when flipped.  Otherwise the same along y: s = (double)(xe -
 *      xs) / dy, (u, v) = ((int)(xs + s t + .5), ys + t).  dx = dy = 0: the one point (xs, ys).  The points of all edges form ONE
 *      sequence in edge order.
 *   3. Every consecutive pair (u', v'), (u, v) of that sequence, across edge boundaries too, with u != u': xd = u < u' ? u : u - 1;
 *      xd = (xd + .5) / 5 - .5; the pair is skipped unless xd is an integer in [0, w - 1]; yd = min(v, v'); yd = (yd + .5) / 5 - .5,
 *      clamped to [0, h], then ceil; toggle at xd h + yd.
 * RLE: `cums` = the cumulative sums of the run lengths (column-major runs, the first a 0-run); a toggle at every cumulative sum (a
 * zero-length run toggles twice at one place).  The host takes the sums, and decodes a compressed `counts` string first.
 * Annotation mask = the OR of its polygons' planes, or its RLE's plane.  Composition per pixel over the image's annotations in
 * list order: persons = OR of every non-crowd mask; miss = OR of the non-crowd masks flagged OG_COCO_MISS (num_keypoints <= 0 or
 * area <= 32 * 32, decided by the host); a crowd annotation at list position c adds crowd' = its mask AND NOT (the OR of the
 * non-crowd masks listed before c); mask_miss = 255 NOT (miss OR crowd'), mask_all = 255 (persons OR crowd').  (The reference raises
 * on a second crowd annotation; here every crowd adds its own crowd'.)  An image without annotations: mask_miss 255, mask_all 0.
 * Tables: one packed buffer, present twice -- tables_host, the bytes as the host wrote them (read by the validation below; pinned or
 * not), and tables_dev, the same bytes on the device (16-byte aligned).  Sections at byte offsets *_at (multiples of 16): images
 * OgCocoImage[n_images]; anns OgCocoAnn[n_anns], image by image; pieces OgCocoPiece[n_pieces], annotation by annotation (a piece =
 * one polygon or one RLE = one bit plane of (h w + 31) / 32 words in the workspace, word_off the running sum); vertices
 * double[2 n_vertices] rows (x, y); cums uint32[n_cums].  Outputs: row-major (h, w) uint8 planes, 0 / 255, image i at byte
 * out_off of mask_miss and of mask_all (device, out_bytes each; mask_all may be NULL) -- the masks / offsets form
 * og_warp_affine_mask_u8 takes.  Four launches (zero the planes, toggle with vector atomic XOR on words -- order-independent, so
 * deterministic --, fill by an in-word shift-XOR prefix and a wave ballot / LDS carry scan, compose one thread per pixel); without
 * pieces only the last.  No allocation, no synchronisation, graph-capturable.
 * og_coco_mask_workspace_bytes: host arithmetic on the descriptor and tables_host (0 for a descriptor og_coco_masks_u8 would refuse).
 * OG_EINVAL (nothing launched): a null pointer; a descriptor of another size; n_images outside 1..65535, a negative count; a
 * section that is misaligned or leaves table_bytes; a non-positive h or w, h w beyond 2^28; planes that leave out_bytes;
 * annotations / pieces / planes that are not consecutive; a piece whose image is not its annotation's; a polygon with fewer than 1
 * vertex, a non-finite vertex, a coordinate beyond 2^20 in magnitude; RLE runs that are negative or do not sum to h w.
 * OG_ENOSPC: workspace_bytes too small. */
#define OG_COCO_POLYGON 0
#define OG_COCO_RLE 1
#define OG_COCO_CROWD 1    /* OgCocoAnn.flags: iscrowd */
#define OG_COCO_MISS 2     /* OgCocoAnn.flags: a person the losses must not see (no keypoints, or area <= 32 * 32) */
typedef struct OgCocoImage {
    int64_t out_off;
    int32_t h, w, ann_first, n_anns;
} OgCocoImage;
typedef struct OgCocoAnn {
    int32_t piece_first, n_pieces, flags, reserved;
} OgCocoAnn;
typedef struct OgCocoPiece {
    int64_t word_off;
    int32_t image, kind, first, count;   /* first / count: rows of `vertices` (polygon) or entries of `cums` (RLE) */
} OgCocoPiece;
typedef struct OgCocoMaskDesc {
    uint32_t size;             /* sizeof(OgCocoMaskDesc): anything else is refused (OG_EINVAL, "descriptor size") */
    int32_t n_images, n_anns, n_pieces, n_vertices, n_cums;
    const void *tables_host;
    const void *tables_dev;
    size_t table_bytes;
    size_t images_at, anns_at, pieces_at, vertices_at, cums_at;
    unsigned char *mask_miss;
    unsigned char *mask_all;
    size_t out_bytes;
    int32_t stages;            /* 0: every launch; else the launches to queue, 1 zero | 2 toggle | 4 fill | 8 compose (for timing them one by one) */
} OgCocoMaskDesc;
size_t og_coco_mask_workspace_bytes(const OgCocoMaskDesc *desc);
int og_coco_masks_u8(const OgCocoMaskDesc *desc, void *workspace, size_t workspace_bytes, void *stream);

/* ---- training step without a host wait (train_dist.py:304-342: the loss.item() batch drop, apex FusedAdam / torch SGD, and
 * torch.nn.utils.clip_grad_norm_; offsetguided_amd.optim.DeviceAdam / DeviceSGD; csrc/optim.hip) ----  A multi-tensor optimizer that
 * reads a device-side gradient scale: the scale carries the clip coefficient and the batch drop, so no step asks the host anything.
 * Tensor table (device memory): `rows` int64[n_rows][5], one row (p, g, m, v, numel) per parameter that has a gradient -- four device
 * addresses of dense fp32 data in one common element order (4-byte aligned, any offset beyond that) and the element count; m is the
 * first moment (Adam) or the momentum buffer (SGD, unused with mom == 0), v the second moment (Adam only).  `chunk_prefix`
 * int32[n_rows + 1] is the running sum of the rows' chunk counts, ceil(numel / og_optim_chunk_elems()), from 0 to the total: workgroup
 * c finds its row by bisection and owns elements (c - chunk_prefix[row]) chunk .. + chunk of it.  A chunk whose offset leaves its row
 * does nothing.  Inside a chunk: 16-byte loads and stores where the address allows (per tensor), scalar head and tail elsewhere.
 * Workspace: a state block [scale f32, norm f32, dropped i32, 4 bytes unused] followed by one double per chunk; 8-byte aligned,
 * og_optim_workspace_bytes(n_chunks) bytes (host arithmetic), owned by the caller across steps (`dropped` accumulates: zero it once).
 * og_grad_sumsq_f32: every gradient element is squared and accumulated in double (an fp32 square is exact in double); partial c =
 * the sum over chunk c in a fixed order (per thread in address order, lanes by a shuffle tree, waves in index order).  No atomics.
 * og_step_scale_f32: ONE workgroup adds the partials in a fixed order (thread t its contiguous share in index order, the thread sums
 * in index order) to n2 and writes the state block:
 *     norm = (float)sqrt(n2)
 *     drop = (loss != NULL && *loss > loss_limit) || !isfinite(n2)
 *     drop:             scale = 0, dropped += 1
 *     finite max_norm:  c = max_norm / (norm + 1e-6f) (fp32);  scale = c < 1 ? c : 1        (torch.nn.utils.clip_grad_norm_)
 *     otherwise:        scale = 1
 * `loss`: device pointer to the weighted fp32 loss, or NULL.  DELIBERATE DIFFERENCE from torch: a non-finite norm (an inf or NaN
 * gradient anywhere) counts as a dropped batch; clip_grad_norm_ would multiply every gradient by NaN and poison every parameter.
 * og_step_scale_amp_f32: og_step_scale_f32 behind a loss scaler (apex amp O1's LossScaler; optim.DeviceLossScaler): the gradients in the
 * table are those of S * loss.  The same reduction in the same order gives n2, the sum of squares of the SCALED gradients.  `scaler`:
 * a 16-byte, 16-byte aligned device block [S f32 (loss_scale), unskipped i32, overflows i32, last_overflow i32], owned by the caller.
 * `loss` is the UNSCALED loss.  It writes the same state words the updates read, so they unscale and clip with one number and skip an
 * overflow step through scale == 0.  Every line ONE rounded operation (fp32 unless it says double):
 *     overflow = !isfinite(n2)
 *     r = sqrt(n2) (double);  q = r / (double)S (double);  norm = (float)q               -- the reported norm is the unscaled one
 *     overflow:             scale = 0;  last_overflow = 1
 *       dynamic:            t = S / scale_factor;  S' = t < min_scale ? min_scale : t;  unskipped' = 0;  overflows += 1
 *                           (`dropped` is NOT counted: a skipped overflow step is the scaler working, not an exploding batch)
 *       static:             dropped += 1                                                 -- og_step_scale_f32's non-finite norm
 *     no overflow:          last_overflow = 0
 *       drop = loss != NULL && *loss > loss_limit
 *       drop:               scale = 0;  dropped += 1
 *       else:               inv = 1.f / S;  c = 1, or with a finite max_norm og_step_scale_f32's c from `norm`;  scale = c * inv
 *       dynamic (dropped or not):  u = unskipped + 1;  if u == scale_window:  t = S * scale_factor;
 *                           S' = t > max_scale ? max_scale : t;  u = 0;  then unskipped' = u
 *   A static scaler (dynamic == 0) leaves S and unskipped alone.  With S a power of two every one of these operations is exact, so a
 *   step on S * g equals the step on g bit for bit; S == 1 static is og_step_scale_f32 (ONE kernel: og_step_scale_f32 launches the
 *   form in which S = 1, static, is a constant and no scaler word is read or written).  apex 0.1's LossScaler defaults: S = 2^16,
 *   scale_factor 2, scale_window 2000, min_scale 1, max_scale 2^24; this text is the specification (bit parity with apex: not pinned).
 *   OG_EINVAL besides og_step_scale_f32's: a null or misaligned scaler block, scale_factor <= 1, scale_window < 1, min_scale <= 0,
 *   max_scale < min_scale, a NaN or infinite one of them.  The block's contents are device memory and are not validated.
 * Updates: ONE launch over chunks chunk_first .. chunk_first + n_chunks of the table (a parameter group, or the parameters of one
 * step count, is a run of rows); scalars by value, computed by the host in double and rounded to fp32 once; `state` = the workspace
 * (scale is read from it) or NULL (scale = 1).  Every line is ONE individually rounded fp32 operation (-ffp-contract=off, correctly
 * rounded divide and sqrt), per element:
 *     ge = (scale == 0) ? 0 : g * scale          -- a dropped batch contributes exactly zero, even where g is inf / NaN
 * og_adam_step_f32 (omb1 = 1 - b1, omb2 = 1 - b2, bc1 = 1 - b1^t, bc2 = 1 - b2^t; adam_w_mode 1 = apex FusedAdam's default, the
 * reference's update; 0 = torch.optim.Adam's L2 form; identical with wd == 0):
 *     if wd != 0 and not adam_w_mode:  t = wd * p;  ge = ge + t
 *     a = b1 * m;   b = omb1 * ge;   m' = a + b
 *     c = b2 * v;   d = omb2 * ge;   e = d * ge;   v' = c + e
 *     mh = m' / bc1
 *     q = v' / bc2;  r = sqrt(q);  den = r + eps
 *     u = mh / den
 *     if wd != 0 and adam_w_mode:      t = wd * p;  u = u + t
 *     s = lr * u;   p' = p - s
 * og_sgd_step_f32 (torch.optim.SGD, dampening 0, no Nesterov):
 *     if wd != 0:  t = wd * p;  ge = ge + t
 *     mom != 0, first:      buf = ge
 *     mom != 0, not first:  t = mom * buf;  buf = t + ge
 *     mom == 0:             buf stands for ge; no buffer is read or written
 *     s = lr * buf;   p' = p - s
 * Weight average (an exponential moving average of the weights, optim.ModelEma; the reference has none: this text is the
 * specification).  og_adam_step_ema_f32 / og_sgd_step_ema_f32 take the arguments of og_adam_step_f32 / og_sgd_step_f32 and
 * `ema`, device memory int64[n_rows] in step with `rows`: the address of the row's average e, or 0 for "this row has none" -- fp32,
 * dense, in the element order of p, 4-byte aligned, any offset beyond that (16-byte accesses where e's own address allows, decided
 * per tensor as for g, m, v; the frame stays p's) -- and omd = 1 - decay of this step, computed by the host in double and rounded to
 * fp32 once.  The p, m, v arithmetic is the list above, unchanged; behind it, with p' the value that is stored, per element, every
 * line ONE individually rounded fp32 operation:
 *     d = p' - e;   t = omd * d;   e' = e + t
 *   A row with ema[r] == 0 runs exactly the plain update and nothing else is read or written.  The average follows p' on EVERY step,
 *   a dropped or overflow step (scale == 0) included: such a step is still the zero-gradient update here (moments decay, weight decay
 *   acts), and the average tracks the weights the model actually has.  A non-finite p' poisons e: not guarded against.  omd == 0
 *   leaves e as it is; omd == 1 gives e + (p' - e), which need not be p'.  The four update entry points launch ONE kernel, instantiated
 *   on its rule (Adam; SGD with or without a buffer) and on the average: og_adam_step_f32 / og_sgd_step_f32 take the form that never
 *   reads `ema`.
 * og_ema_lerp_f32: the same three lines with x for p', for the tensors no update touches in a step (BatchNorm running statistics,
 * frozen parameters, a parameter without a gradient).  Table: `rows` int64[n_rows][3], one row (e, x, numel) -- two device addresses
 * of dense fp32 data in one common element order, 4-byte aligned, any offset beyond that; e is read and written, x read -- and the
 * chunk prefix as above, chunks of og_optim_chunk_elems() elements.  The frame is e's; x takes 16-byte loads where its address allows.
 * All: no allocation, no synchronisation, graph-capturable; n_chunks == 0 launches nothing (og_step_scale_f32 always launches).
 * OG_EINVAL (nothing launched): a null or misaligned table, workspace, loss or state; n_rows <= 0; a negative chunk count; a NaN
 * max_norm or loss_limit; bc1 or bc2 not positive; for the _ema entry points and og_ema_lerp_f32 a null or misaligned (8 bytes) `ema`
 * table, omd outside [0, 1] or NaN.  OG_ENOSPC: workspace_bytes too small.  The tables' contents are device memory and are not
 * validated: their builder answers for addresses and counts. */
int og_optim_chunk_elems(void);
size_t og_optim_workspace_bytes(int n_chunks);
int og_grad_sumsq_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int n_chunks, void *workspace,
                      size_t workspace_bytes, void *stream);
int og_step_scale_f32(int n_chunks, const float *loss, float loss_limit, float max_norm, void *workspace, size_t workspace_bytes,
                      void *stream);
int og_step_scale_amp_f32(int n_chunks, const float *loss, float loss_limit, float max_norm, void *scaler, int dynamic,
                          float scale_factor, int scale_window, float min_scale, float max_scale, void *workspace,
                          size_t workspace_bytes, void *stream);
int og_adam_step_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks, const void *state,
                     float lr, float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1, float bc2, int adam_w_mode,
                     void *stream);
int og_sgd_step_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks, const void *state,
                    float lr, float mom, float wd, int first, void *stream);
int og_adam_step_ema_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks, const void *state,
                         float lr, float b1, float b2, float omb1, float omb2, float eps, float wd, float bc1, float bc2,
                         int adam_w_mode, const int64_t *ema, float omd, void *stream);
int og_sgd_step_ema_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int chunk_first, int n_chunks, const void *state,
                        float lr, float mom, float wd, int first, const int64_t *ema, float omd, void *stream);
int og_ema_lerp_f32(const int64_t *rows, const int32_t *chunk_prefix, int n_rows, int n_chunks, float omd, void *stream);

/* ---- weight refresh: BatchNorm fold + 16-bit cast of every layer in one launch (models/engine.py: InferenceEngine.refresh;
 * csrc/fold.hip) ----  What an engine computes with torch ops when it is built (_fold, .to(dtype), channels-last), written into the
 * buffers it already has, so that captured graphs keep their addresses.  Table (device memory, filled by the caller in pinned memory
 * and copied once): `rows` int64[n_rows][og_fold_row_words() = 16], one row per convolution:
 *     [0] w       fp32 weight (Cout, Cin, kh, kw), dense; 4-byte aligned, any offset beyond that
 *     [1] bias    fp32 (Cout) or 0
 *     [2..5]      BatchNorm weight (gamma), bias (beta), running_mean, running_var, fp32 (Cout) each; all four or all 0 (no BN)
 *     [6] dst w   16-bit (Cout, kh, kw, Cin): the memory of a channels-last (Cout, Cin, kh, kw) tensor
 *     [7] dst b32 fp32 (Cout) or 0      [8] dst b  16-bit (Cout) or 0
 *     [9] Cout    [10] Cin    [11] kh * kw    [12] bit 0: the source's memory is channels-last ((Cout, kh, kw, Cin)), else OIHW
 *     [13] eps    the fp32 bit pattern of the BatchNorm's eps (the double rounded once)
 *     [14] partner  row whose b' is added to this row's (same Cout), or -1: the layer whose output meets this one's before the
 *                 activation (a residual's projection on conv2, the junction's cnvs_ on inters_)
 *     [15] slab   output channels per workgroup (> 0); the row has ceil(Cout / slab) workgroups
 * `wg_prefix` int32[n_rows + 1]: the running sum of the rows' workgroup counts from 0 to n_workgroups.  The rule, per output channel
 * o, every line ONE rounded fp32 operation (-ffp-contract=off, correctly rounded divide and sqrt):
 *     s = var[o] + eps;  r = sqrt(s);  scale = gamma[o] / r            (no BN: no scale, w' = w, b' = bias or 0)
 *     w' = w * scale                    then round-to-nearest-even to the 16-bit type
 *     d = bias[o] - mean[o] (bias = 0 without one);  m = d * scale;  b' = m + beta[o]
 *     partner:  b' = b'(this row) + b'(partner row)
 *     dst b32 = b';  dst b = b' rounded to the 16-bit type
 * f16 != 0: fp16 (a value beyond its range becomes inf, as torch's cast; subnormals are kept), else bf16 (a NaN becomes 0x7fc0), for
 * the whole launch.  A workgroup reads each output channel's weights as one contiguous run (16-byte loads where the address allows)
 * and writes 16-byte stores where dst w is 16-byte aligned and Cin (channels-last source or 1x1: Cin * kh * kw) is a multiple of 8;
 * an OIHW source is permuted through LDS.  A row with more than 512 taps, or whose workgroup falls outside it, is left alone.  No
 * allocation, no synchronisation.  OG_EINVAL (nothing launched): a null or misaligned table, n_rows <= 0, a negative workgroup
 * count.  The table's contents are device memory and are not validated: its builder answers for addresses, shapes and counts. */
int og_fold_row_words(void);
int og_fold_bn_w16(const int64_t *rows, const int32_t *wg_prefix, int n_rows, int n_workgroups, int f16, void *stream);

/* ---- range report: what the engine's 16-bit type does to a tensor, counted on the device (models/range_report.py,
 * InferenceEngine.weight_report / probe=True; csrc/range.hip) ----  A stats row is OG_RANGE_WORDS = 9 int64 words that every call
 * ACCUMULATES into; a row of zeros is the identity (a fresh row is zeros).  For an element x of source type S (OG_RANGE_F32 /
 * OG_RANGE_F16 / OG_RANGE_BF16) and the target type T (OG_RANGE_F16 / OG_RANGE_BF16; S is fp32 or T): y = x rounded to T, to nearest
 * even, subnormals kept -- the cast of og_fold_bn_w16 -- and y = x when S = T.  Every class is decided on BIT PATTERNS with integer
 * comparisons (abs = the pattern without its sign; a 16-bit source is widened to fp32 exactly), so no denormal mode changes a count:
 *     [0] n      elements seen
 *     [1] nan    x is a NaN (any payload)
 *     [2] inf    x is +-inf
 *     [3] over   x finite, y = +-inf       fp16: |x| >= 65520 (abs >= 0x477ff000);  bf16: abs >= 0x7f7f8000;  0 when S = T
 *     [4] zero   x = +-0
 *     [5] flush  x != 0, y = +-0           fp16: |x| <= 2^-25 (abs <= 0x33000000);  bf16: abs <= 0x00008000;  0 when S = T
 *     [6] sub    y is a non-zero subnormal of T    fp16: 2^-25 < |x| < 1023.5 * 2^-24 (the tie rounds to the normal 2^-14)
 *     [7] max    max over finite x of the fp32 bit pattern of |x|
 *     [8] min    max over finite non-zero x of 0x7f800000 - (fp32 bit pattern of |x|): 0 = none seen, else the smallest non-zero
 *                magnitude is the fp32 whose pattern is 0x7f800000 - [8]
 * Words 0..6 are sums and words 7, 8 maxima: the result does not depend on any order, is exact and the same on every run.
 * og_range_stats: a table in device memory, `rows` int64[n_rows][4] = [pointer, numel, source type, stats row index], and
 * `wg_prefix` int32[n_rows + 1], the running sum of the rows' workgroup counts from 0 to n_workgroups; a row's workgroups share its
 * chunks of og_range_chunk_elems() elements in turn (a row needs at most ceil(numel / chunk) of them, a row of no elements none).
 * Several table rows may name one stats row; `stats` int64[.][9] holds every row the table names.  One launch.
 * og_range_probe: one tensor whose pointer and size are kernel arguments (inside a graph capture a tensor's address is not the one
 * of the warm-up passes: a device table would have to be rewritten), into the one row `stats_row`.
 * Both: tensors are dense runs of numel elements, aligned to their element size, any offset beyond that (16-byte loads between a
 * scalar head and tail; nothing outside the run is read); numel = 0 touches nothing; no allocation, no workspace, no
 * synchronisation, graph-capturable.  OG_EINVAL (nothing launched): a null or misaligned table, stats or tensor; n_rows <= 0; a
 * negative count; a target that is not a 16-bit type; og_range_probe: a source that is neither fp32 nor the target.  The table's
 * contents are device memory and are not validated: its builder answers for addresses, counts and stats row indices; a table row
 * whose source type the launch does not serve is passed over. */
#define OG_RANGE_WORDS 9
#define OG_RANGE_F32 0
#define OG_RANGE_F16 1
#define OG_RANGE_BF16 2
int og_range_chunk_elems(void);
int og_range_stats(const int64_t *rows, const int32_t *wg_prefix, int n_rows, int n_workgroups, int target, int64_t *stats,
                   void *stream);
int og_range_probe(const void *x, int64_t numel, int source, int target, int64_t *stats_row, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* OG_DECODER_H */
