// Multi-scale test: one scale's head outputs resampled onto the base grid and accumulated (decoder/multiscale.py).
//
// Per base cell (j, i) of image n, with the host's affine table aff[n] = (Ax, Bx, Ay, By, inv_ax, inv_ay):
//   u = clamp(Ax*j + Bx, 0, ws-1), x0 = floor(u), x1 = min(x0+1, ws-1), fx = u - x0     (rows alike with Ay, By, hs)
//   top = p00*(1-fx) + p01*fx, bot = p10*(1-fx) + p11*fx, v = top*(1-fy) + bot*fy
//   offsets: v *= inv_ax (x components, even channels) / inv_ay (y components, odd channels); heatmaps as they are
//   mode 0: acc = v, 1: acc = acc + v, 2: acc = (acc + v) * inv_count
// With flip the input is the [images | mirrored images] pair: every tap reads the value og_flip_merge_f32 would have written at
// that source cell ((a + flipW(b)[perm]) / 2, x offsets negated, reserve limbs un-averaged), so the result is bit-identical to
// og_flip_merge_f32 followed by the resample, without the merged maps ever being stored.  fp32 throughout, no contraction
// (-ffp-contract=off).  Every index is clamped into the source plane whatever the table holds.
//
// og_scale_accumulate_heads_f32: the same launch over the channel list [hm | off | scale | jitter] (HEADS instantiation; the two-map
// kernel is instantiated without it and is unchanged).  Keypoint-scale planes (N, C, hs, ws) merge under flip as the heat maps do
// (mirror, kp_perm, average) and are a length in scale-s input pixels: v *= sqrtf(inv_ax * inv_ay) (one multiply, one correctly
// rounded square root).  Jitter planes (N, 2, hs, ws) merge as og_flip_merge_heads_f32 merges them (mirror, x channel negated,
// average, no permutation) and are offsets: v *= inv_ax (channel 0) / inv_ay (channel 1).
#include "og_common.h"

namespace {

struct Src {
    const float *a, *b;   // the image's plane; with flip the mirrored image's (permuted) plane, else null
    float sign;           // x offsets change sign in the mirror
    bool keep;            // reserve limb: the un-averaged original
};

__device__ __forceinline__ float tap(const Src &s, int ws, int y, int x)
{
    const float av = s.a[(size_t)y * ws + x];
    if (!s.b || s.keep) return av;
    const float fv = s.b[(size_t)y * ws + (ws - 1 - x)] * s.sign;
    return (av + fv) / 2.f;
}

struct Heads {           // the optional maps of the HEADS form; a head that is absent has 0 channels
    const float *scl, *jit;
    float *scl_acc, *jit_acc;
    int C_sc, C_jo;
};

template <bool HEADS>
__global__ void __launch_bounds__(256)
scale_accumulate_kernel(const float *__restrict__ hm, const float *__restrict__ off, int N, int flip, int C, int L, int hs, int ws,
                        const int32_t *__restrict__ kp_perm, const int32_t *__restrict__ limb_perm,
                        const int32_t *__restrict__ reserve, const float *__restrict__ aff, int h, int w, int mode, float inv_count,
                        float *__restrict__ hm_acc, float *__restrict__ off_acc, Heads hd)
{
    const int planes_per_img = C + 2 * L + (HEADS ? hd.C_sc + hd.C_jo : 0);
    const int plane = blockIdx.y;  // (n, channel) over the concatenated [hm | off] channel list
    const int n = plane / planes_per_img, ch = plane % planes_per_img;
    const size_t hws = (size_t)hs * ws, hw = (size_t)h * w;
    Src s{nullptr, nullptr, 1.f, false};
    float unit = 1.f;
    float *o;
    const float *t = aff + (size_t)n * 6;
    const float Ax = t[0], Bx = t[1], Ay = t[2], By = t[3];
    if (ch < C) {
        s.a = hm + ((size_t)n * C + ch) * hws;
        if (flip) s.b = hm + ((size_t)(n + N) * C + kp_perm[ch]) * hws;
        o = hm_acc + ((size_t)n * C + ch) * hw;
    } else if (!HEADS || ch < C + 2 * L) {
        const int oc = ch - C, l = oc >> 1, comp = oc & 1;
        s.a = off + ((size_t)n * 2 * L + oc) * hws;
        if (flip) {
            s.b = off + ((size_t)(n + N) * 2 * L + 2 * limb_perm[l] + comp) * hws;
            s.sign = comp == 0 ? -1.f : 1.f;
            s.keep = reserve[l] != 0;
        }
        unit = comp == 0 ? t[4] : t[5];
        o = off_acc + ((size_t)n * 2 * L + oc) * hw;
    } else if (ch < C + 2 * L + hd.C_sc) {
        const int sc = ch - C - 2 * L;
        s.a = hd.scl + ((size_t)n * hd.C_sc + sc) * hws;
        if (flip) s.b = hd.scl + ((size_t)(n + N) * hd.C_sc + kp_perm[sc]) * hws;
        const float area = t[4] * t[5];
        unit = sqrtf(area);
        o = hd.scl_acc + ((size_t)n * hd.C_sc + sc) * hw;
    } else {
        const int jc = ch - C - 2 * L - hd.C_sc;
        s.a = hd.jit + ((size_t)n * hd.C_jo + jc) * hws;
        if (flip) {
            s.b = hd.jit + ((size_t)(n + N) * hd.C_jo + jc) * hws;
            s.sign = jc == 0 ? -1.f : 1.f;
        }
        unit = jc == 0 ? t[4] : t[5];
        o = hd.jit_acc + ((size_t)n * hd.C_jo + jc) * hw;
    }
    const float xmax = (float)(ws - 1), ymax = (float)(hs - 1);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) {
        const int yi = (int)(i / w), xj = (int)(i % w);
        float u = Ax * (float)xj;
        u = u + Bx;
        u = fminf(fmaxf(u, 0.f), xmax);
        float r = Ay * (float)yi;
        r = r + By;
        r = fminf(fmaxf(r, 0.f), ymax);
        const int x0 = (int)floorf(u), y0 = (int)floorf(r);
        const int x1 = min(x0 + 1, ws - 1), y1 = min(y0 + 1, hs - 1);
        const float fx = u - (float)x0, fy = r - (float)y0;
        const float gx = 1.f - fx, gy = 1.f - fy;
        const float p00 = tap(s, ws, y0, x0), p01 = tap(s, ws, y0, x1);
        const float p10 = tap(s, ws, y1, x0), p11 = tap(s, ws, y1, x1);
        const float top = p00 * gx + p01 * fx;
        const float bot = p10 * gx + p11 * fx;
        float v = top * gy + bot * fy;
        if (ch >= C) v = v * unit;
        if (mode == 0) {
            o[i] = v;
        } else {
            const float acc = o[i] + v;
            o[i] = mode == 2 ? acc * inv_count : acc;
        }
    }
}

int scale_accumulate(const char *name, const float *hm, const float *off, const Heads *hd, int N, int flip, int C, int L, int hs, int ws,
                     const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask, const float *aff, int h, int w,
                     int mode, float inv_count, float *hm_acc, float *off_acc, void *stream)
{
    OG_REQUIRE(hm && off && aff && hm_acc && off_acc, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(!flip || (kp_perm && limb_perm && reserve_mask), OG_EINVAL, "%s: null pointer (flip tables)", name);
    OG_REQUIRE(N > 0 && C > 0 && L > 0 && hs > 0 && ws > 0 && h > 0 && w > 0, OG_EINVAL, "%s: bad shape", name);
    OG_REQUIRE(mode >= 0 && mode <= 2, OG_EINVAL, "%s: mode %d (0 write, 1 add, 2 add and scale)", name, mode);
    const long planes = (long)N * (C + 2 * L + (hd ? hd->C_sc + hd->C_jo : 0));
    OG_REQUIRE(planes <= 65535, OG_EINVAL, "%s: too many planes", name);
    const size_t blocks = ((size_t)h * w + 255) / 256;
    const dim3 grid(blocks < 128 ? (unsigned)blocks : 128u, (unsigned)planes);
    if (hd)
        hipLaunchKernelGGL(scale_accumulate_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, hm, off, N, flip ? 1 : 0, C, L, hs, ws,
                           kp_perm, limb_perm, reserve_mask, aff, h, w, mode, inv_count, hm_acc, off_acc, *hd);
    else
        hipLaunchKernelGGL(scale_accumulate_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, hm, off, N, flip ? 1 : 0, C, L, hs,
                           ws, kp_perm, limb_perm, reserve_mask, aff, h, w, mode, inv_count, hm_acc, off_acc, Heads{});
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

}  // namespace

OG_API int og_scale_accumulate_f32(const float *hm, const float *off, int N, int flip, int C, int L, int hs, int ws,
                                   const int32_t *kp_perm, const int32_t *limb_perm, const int32_t *reserve_mask,
                                   const float *aff, int h, int w, int mode, float inv_count, float *hm_acc, float *off_acc,
                                   void *stream)
{
    return scale_accumulate("og_scale_accumulate_f32", hm, off, nullptr, N, flip, C, L, hs, ws, kp_perm, limb_perm, reserve_mask, aff, h,
                            w, mode, inv_count, hm_acc, off_acc, stream);
}

OG_API int og_scale_accumulate_heads_f32(const float *hm, const float *off, const float *scl, const float *jit, int N, int flip, int C,
                                         int L, int hs, int ws, const int32_t *kp_perm, const int32_t *limb_perm,
                                         const int32_t *reserve_mask, const float *aff, int h, int w, int mode, float inv_count,
                                         float *hm_acc, float *off_acc, float *scl_acc, float *jit_acc, void *stream)
{
    const char *name = "og_scale_accumulate_heads_f32";
    OG_REQUIRE((scl == nullptr) == (scl_acc == nullptr) && (jit == nullptr) == (jit_acc == nullptr), OG_EINVAL,
               "%s: null pointer (every head needs its accumulator, and no accumulator without its head)", name);
    const Heads hd{scl, jit, scl_acc, jit_acc, scl ? C : 0, jit ? 2 : 0};
    return scale_accumulate(name, hm, off, &hd, N, flip, C, L, hs, ws, kp_perm, limb_perm, reserve_mask, aff, h, w, mode, inv_count,
                            hm_acc, off_acc, stream);
}
