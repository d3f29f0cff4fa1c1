// K0 -- PostProcess.flip_augment, vector-addition form (decoder/factory.py:98-146).
//
//   hm  = (hm[:N]  + flipW(hm[N:])[:, kp_perm]) / 2
//   off = (off[:N] + flipW(off[N:] with x components negated)[:, limb_perm]) / 2,
//         except limbs whose mirror image is their own reverse ({2,5,14} for COCO), which keep
//         the un-averaged original.
// One elementwise pass over the stride-4 maps (the reference makes ~8); exact in fp32.
//
// cat_flip_offs form (factory.py:115-127): the mirrored offsets are appended as components 2,3 of a
// (N, L, 4, h, w) tensor instead of being averaged (reserve limbs repeat their own components there).
#include "og_common.h"

namespace {

__global__ void __launch_bounds__(256)
flip_merge_kernel(const float *__restrict__ hm, const float *__restrict__ off, int N, int C, int L, int h, int w,
                  const int32_t *__restrict__ kp_perm, const int32_t *__restrict__ limb_perm,
                  const int32_t *__restrict__ reserve, float *__restrict__ hm_out, float *__restrict__ off_out, int cat)
{
    const int planes_per_img = C + 2 * L;
    const int plane = blockIdx.y;  // (n, channel) over the concatenated [hm | off] channel list
    const int n = plane / planes_per_img, ch = plane % planes_per_img;
    const size_t hw = (size_t)h * w;
    const float *a, *b;
    float *o, *o2 = nullptr;
    float sign = 1.f;
    bool keep = false;
    if (ch < C) {
        a = hm + ((size_t)n * C + ch) * hw;
        b = hm + ((size_t)(n + N) * C + kp_perm[ch]) * hw;
        o = hm_out + ((size_t)n * C + ch) * hw;
    } else {
        const int oc = ch - C, l = oc >> 1, comp = oc & 1;
        a = off + ((size_t)n * 2 * L + oc) * hw;
        b = off + ((size_t)(n + N) * 2 * L + 2 * limb_perm[l] + comp) * hw;
        o = off_out + ((size_t)n * 2 * L + oc) * hw;
        if (cat) {
            o = off_out + ((size_t)n * 4 * L + 4 * l + comp) * hw;
            o2 = o + 2 * hw;
        }
        sign = comp == 0 ? -1.f : 1.f;
        keep = reserve[l] != 0;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i % w);
        const float av = a[i];
        const float fv = b[(size_t)y * w + (w - 1 - x)] * sign;
        if (o2) {
            o[i] = av;
            o2[i] = keep ? av : fv;
        } else {
            o[i] = keep ? av : (av + fv) / 2.f;
        }
    }
}

// The two optional heads of flip_augment in the same vector-addition form (decoder/factory.py:108-113, :141-144):
//   scale  = (sc[:N] + flipW(sc[N:])[:, kp_perm]) / 2
//   jitter = (jo[:N] + flipW(jo[N:] with the even = x channel negated)) / 2      (no permutation: two channels shared by all joints)
// Planes are the concatenated [scale | jitter] channel list of an image; either map may be absent (C_sc or C_jo = 0).
__global__ void __launch_bounds__(256)
flip_merge_heads_kernel(const float *__restrict__ sc, const float *__restrict__ jo, int N, int C_sc, int C_jo, int h, int w,
                        const int32_t *__restrict__ kp_perm, float *__restrict__ sc_out, float *__restrict__ jo_out)
{
    const int planes_per_img = C_sc + C_jo;
    const int plane = blockIdx.y;
    const int n = plane / planes_per_img, ch = plane % planes_per_img;
    const size_t hw = (size_t)h * w;
    const float *a, *b;
    float *o;
    float sign = 1.f;
    if (ch < C_sc) {
        a = sc + ((size_t)n * C_sc + ch) * hw;
        b = sc + ((size_t)(n + N) * C_sc + kp_perm[ch]) * hw;
        o = sc_out + ((size_t)n * C_sc + ch) * hw;
    } else {
        const int jc = ch - C_sc;
        a = jo + ((size_t)n * C_jo + jc) * hw;
        b = jo + ((size_t)(n + N) * C_jo + jc) * hw;
        o = jo_out + ((size_t)n * C_jo + jc) * hw;
        sign = (jc & 1) == 0 ? -1.f : 1.f;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i % w);
        o[i] = (a[i] + b[(size_t)y * w + (w - 1 - x)] * sign) / 2.f;
    }
}

}  // namespace

OG_API int og_flip_merge_heads_f32(const float *scmps, const float *jomps, int N, int C, int h, int w, const int32_t *kp_perm,
                                   float *sc_out, float *jo_out, void *stream)
{
    const char *name = "og_flip_merge_heads_f32";
    OG_REQUIRE(scmps || jomps, OG_EINVAL, "%s: null pointer (neither head given)", name);
    OG_REQUIRE((scmps == nullptr) == (sc_out == nullptr) && (jomps == nullptr) == (jo_out == nullptr), OG_EINVAL,
               "%s: null pointer (every head needs its output, and no output without its head)", name);
    OG_REQUIRE(!scmps || kp_perm, OG_EINVAL, "%s: null pointer (kp_perm)", name);
    OG_REQUIRE(N > 0 && h > 0 && w > 0 && (!scmps || C > 0), OG_EINVAL, "%s: bad shape", name);
    const int C_sc = scmps ? C : 0, C_jo = jomps ? 2 : 0;
    const long planes = (long)N * (C_sc + C_jo);
    OG_REQUIRE(planes <= 65535, OG_EINVAL, "%s: too many planes", name);
    const int bx = (int)(((size_t)h * w + 255) / 256);
    hipLaunchKernelGGL(flip_merge_heads_kernel, dim3(bx < 64 ? bx : 64, (unsigned)planes), dim3(256), 0, (hipStream_t)stream, scmps,
                       jomps, N, C_sc, C_jo, h, w, kp_perm, sc_out, jo_out);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

static int flip_launch(const char *name, int cat, const float *hm, const float *off, int N, int C, int L, int h, int w,
                       const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask, float *hm_out,
                       float *off_out, void *stream)
{
    OG_REQUIRE(hm && off && kp_perm && limb_perm && reserve_mask && hm_out && off_out, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && L > 0 && h > 0 && w > 0, OG_EINVAL, "%s: bad shape", name);
    const long planes = (long)N * (C + 2 * L);
    OG_REQUIRE(planes <= 65535, OG_EINVAL, "%s: too many planes", name);
    const int bx = (int)(((size_t)h * w + 255) / 256);
    hipLaunchKernelGGL(flip_merge_kernel, dim3(bx < 64 ? bx : 64, (unsigned)planes), dim3(256), 0, (hipStream_t)stream, hm,
                       off, N, C, L, h, w, kp_perm, limb_perm, reserve_mask, hm_out, off_out, cat);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_flip_merge_f32(const float *hm, const float *off, int N, int C, int L, int h, int w,
                             const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask,
                             float *hm_out, float *off_out, void *stream)
{
    return flip_launch("og_flip_merge_f32", 0, hm, off, N, C, L, h, w, kp_perm, limb_perm, reserve_mask, hm_out, off_out,
                       stream);
}

OG_API int og_flip_cat_f32(const float *hm, const float *off, int N, int C, int L, int h, int w,
                           const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask,
                           float *hm_out, float *off_out, void *stream)
{
    return flip_launch("og_flip_cat_f32", 1, hm, off, N, C, L, h, w, kp_perm, limb_perm, reserve_mask, hm_out, off_out,
                       stream);
}
