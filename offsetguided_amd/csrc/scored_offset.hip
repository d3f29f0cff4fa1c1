// Heatmap-weighted offset refinement (reference decoder/offset.py:8-43; PostProcess calls it with kernel_size 3,
// decoder/factory.py:70-72) as one streaming pass over the stride-4 maps:
//
//   out[n, 2l+c] = box_ks(hm[n, jf[l]] * off[n, 2l+c]) / (box_ks(hm[n, jf[l]]) + 1e-6)
//
// with the fp32 rounding of the torch-CPU formulation (avg_pool2d with divisor_override=1): every product is rounded
// before any sum, both box sums start at +0 and add the in-bounds cells row-major (y' outer, x' inner), one after the
// other.  Cells outside the plane enter the LDS tile as zeros instead of being skipped: a sum that starts at +0 is never
// -0 (x + -x and +0 + -0 round to +0), so adding +0 (0 * 0, the stored product there) changes no bit pattern, NaN and Inf
// of in-bounds cells included.
//
// One workgroup per (image, limb, row band[, column tile]).  The band of the heat-map plane and of the two product planes
// plus a p-row halo is staged in LDS once -- every input element is fetched once per (n, l) apart from the halo rows (planes
// wider than 256 columns are cut into column tiles, whose p halo columns are fetched twice as well) -- and each thread
// produces 4 neighbouring cells of a row from a (ks x (4 + 2p)) register window per plane; the denominator is computed
// once for both components.  16-byte global loads and stores when w % 4 == 0 and the pointers are 16-byte aligned.
#include "og_common.h"

namespace {

constexpr int kPadL = 4;               // zero columns left of the tile in LDS (>= p; 4 keeps the 16-byte alignment of a row)
constexpr int kMaxTileW = 256;
constexpr size_t kLdsBudget = 48 * 1024;

template <int KS, bool VEC4>
__global__ void __launch_bounds__(256)
scored_offset_kernel(const float *__restrict__ hm, const float *__restrict__ off, int C, int L, int h, int w,
                     const int32_t *__restrict__ jf, float *__restrict__ out, int TH, int TW, int bands, int ctiles)
{
    constexpr int P = (KS - 1) / 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int b = blockIdx.x;
    const int ct = b % ctiles;
    b /= ctiles;
    const int band = b % bands;
    b /= bands;
    const int l = b % L, n = b / L;
    const int cf = jf[l];
    if ((unsigned)cf >= (unsigned)C) return;        // a joint table that does not fit the heat maps: nothing is read or written
    const int y0 = band * TH, x0 = ct * TW;
    const int th = min(TH, h - y0), tw = min(TW, w - x0);
    const int SW = TW + 2 * kPadL, rows = th + 2 * P, plane = (TH + 2 * P) * SW;
    float *sh = lds, *s0 = lds + plane, *s1 = lds + 2 * plane;
    const size_t hw = (size_t)h * w;
    const float *ph = hm + ((size_t)n * C + cf) * hw;
    const float *p0 = off + ((size_t)n * 2 * L + 2 * l) * hw, *p1 = p0 + hw;

    // LDS cell (r, j) <-> plane cell (y0 - P + r, x0 - kPadL + j); groups of 4 columns
    const int groups = SW / 4;
    for (int i = threadIdx.x; i < rows * groups; i += 256) {
        const int r = i / groups, g = i % groups;
        const int gy = y0 - P + r, gx = x0 - kPadL + 4 * g;
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f), a = m, c = m;
        if (gy >= 0 && gy < h) {
            const size_t base = (size_t)gy * w;
            if (VEC4) {     // w % 4 == 0 and gx % 4 == 0: a group lies inside the row or outside it
                if (gx >= 0 && gx < w) {
                    m = *reinterpret_cast<const float4 *>(ph + base + gx);
                    a = *reinterpret_cast<const float4 *>(p0 + base + gx);
                    c = *reinterpret_cast<const float4 *>(p1 + base + gx);
                }
            } else {
                float mv[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f}, cv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gx + j >= 0 && gx + j < w) {
                        mv[j] = ph[base + gx + j];
                        av[j] = p0[base + gx + j];
                        cv[j] = p1[base + gx + j];
                    }
                m = make_float4(mv[0], mv[1], mv[2], mv[3]);
                a = make_float4(av[0], av[1], av[2], av[3]);
                c = make_float4(cv[0], cv[1], cv[2], cv[3]);
            }
        }
        const int o = r * SW + 4 * g;
        *reinterpret_cast<float4 *>(sh + o) = m;
        *reinterpret_cast<float4 *>(s0 + o) = make_float4(m.x * a.x, m.y * a.y, m.z * a.z, m.w * a.w);   // rounded products
        *reinterpret_cast<float4 *>(s1 + o) = make_float4(m.x * c.x, m.y * c.y, m.z * c.z, m.w * c.w);
    }
    __syncthreads();

    float *o0 = out + ((size_t)n * 2 * L + 2 * l) * hw, *o1 = o0 + hw;
    const int strips = TW / 4;
    for (int i = threadIdx.x; i < th * strips; i += 256) {
        const int r = i / strips, x = 4 * (i % strips);
        if (x >= tw) continue;
        float den[4] = {0.f, 0.f, 0.f, 0.f}, n0[4] = {0.f, 0.f, 0.f, 0.f}, n1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < KS; ++dy) {
            const int o = (r + dy) * SW + kPadL + x - P;
            float vh[4 + 2 * P], v0[4 + 2 * P], v1[4 + 2 * P];
#pragma unroll
            for (int j = 0; j < 4 + 2 * P; ++j) {
                vh[j] = sh[o + j];
                v0[j] = s0[o + j];
                v1[j] = s1[o + j];
            }
#pragma unroll
            for (int dx = 0; dx < KS; ++dx)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    den[j] += vh[j + dx];
                    n0[j] += v0[j + dx];
                    n1[j] += v1[j + dx];
                }
        }
        float r0[4], r1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = den[j] + 1e-6f;
            r0[j] = n0[j] / d;
            r1[j] = n1[j] / d;
        }
        const size_t go = (size_t)(y0 + r) * w + x0 + x;
        if (VEC4) {
            *reinterpret_cast<float4 *>(o0 + go) = make_float4(r0[0], r0[1], r0[2], r0[3]);
            *reinterpret_cast<float4 *>(o1 + go) = make_float4(r1[0], r1[1], r1[2], r1[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < tw) {
                    o0[go + j] = r0[j];
                    o1[go + j] = r1[j];
                }
        }
    }
}

template <int KS>
void launch(bool vec4, dim3 grid, size_t lds, hipStream_t stream, const float *hm, const float *off, int C, int L, int h, int w,
            const int32_t *jf, float *out, int TH, int TW, int bands, int ctiles)
{
    if (vec4)
        hipLaunchKernelGGL((scored_offset_kernel<KS, true>), grid, dim3(256), lds, stream, hm, off, C, L, h, w, jf, out, TH, TW, bands,
                           ctiles);
    else
        hipLaunchKernelGGL((scored_offset_kernel<KS, false>), grid, dim3(256), lds, stream, hm, off, C, L, h, w, jf, out, TH, TW, bands,
                           ctiles);
}

}  // namespace

OG_API int og_scored_offset_f32(const float *hm, const float *off, int N, int C, int L, int h, int w, const int32_t *jf, int ksize,
                                float *out, void *stream)
{
    const char *name = "og_scored_offset_f32";
    OG_REQUIRE(ksize == 1 || ksize == 3 || ksize == 5 || ksize == 7, OG_EINVAL, "%s: ksize must be odd, 1..7 (got %d)", name, ksize);
    OG_REQUIRE(hm && off && jf && out, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && L > 0 && h > 0 && w > 0, OG_EINVAL, "%s: bad shape", name);
    OG_REQUIRE(out != off, OG_EINVAL, "%s: out must not alias off", name);
    OG_REQUIRE((long)h * w < (1l << 31), OG_EINVAL, "%s: plane too large", name);
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, jf) == hipSuccess && attr.type == hipMemoryTypeHost && attr.hostPointer) {
        const int32_t *t = static_cast<const int32_t *>(attr.hostPointer);   // a pinned (host-visible) table can be checked here
        for (int l = 0; l < L; ++l)
            OG_REQUIRE(t[l] >= 0 && t[l] < C, OG_EINVAL, "%s: jf[%d] = %d outside [0, %d)", name, l, t[l], C);
    } else {
        (void)hipGetLastError();    // (a pointer the runtime does not know is not an error of this call)
    }
    const int p = (ksize - 1) / 2;
    const int TW = min((w + 3) / 4 * 4, kMaxTileW), ctiles = (w + TW - 1) / TW;
    const int rows_max = (int)(kLdsBudget / (3 * sizeof(float) * (TW + 2 * kPadL)));    // >= 15 > 2p + 1
    const int bands = (h + (rows_max - 2 * p) - 1) / (rows_max - 2 * p), TH = (h + bands - 1) / bands;
    const long total = (long)N * L * bands * ctiles;
    OG_REQUIRE(total < (1l << 31), OG_EINVAL, "%s: too many work items", name);
    const size_t lds = (size_t)3 * (TH + 2 * p) * (TW + 2 * kPadL) * sizeof(float);
    const bool vec4 = w % 4 == 0 && (uintptr_t)hm % 16 == 0 && (uintptr_t)off % 16 == 0 && (uintptr_t)out % 16 == 0;
    const dim3 grid((unsigned)total);
    hipStream_t st = (hipStream_t)stream;
    switch (ksize) {
    case 1: launch<1>(vec4, grid, lds, st, hm, off, C, L, h, w, jf, out, TH, TW, bands, ctiles); break;
    case 3: launch<3>(vec4, grid, lds, st, hm, off, C, L, h, w, jf, out, TH, TW, bands, ctiles); break;
    case 5: launch<5>(vec4, grid, lds, st, hm, off, C, L, h, w, jf, out, TH, TW, bands, ctiles); break;
    default: launch<7>(vec4, grid, lds, st, hm, off, C, L, h, w, jf, out, TH, TW, bands, ctiles); break;
    }
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
