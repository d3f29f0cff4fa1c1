// Model-inspection views painted over a uint8 RGB batch in place (visualization/__init__.py: draw_heatmap, draw_segments, draw_limbs,
// draw_offsets; evaluate.py --show-hmp-idx / --show-all-limbs / --show-limb-idx).  The semantics of the entry points are spelled out in
// include/og_decoder.h.
//
//   heatmap overlay   one 256-thread workgroup per tile of 64 x 16 pixels of image blockIdx.z, four pixels per thread (rows 4 apart: a
//                     wave writes 192 contiguous bytes).  The hi-res value of a pixel is og_bicubic4_at on the stride-4 plane: the
//                     x4 plane is never built.  With NMS the tile's values and a one-pixel halo (66 x 18, zero outside the image) are
//                     computed once into LDS (4.6 KiB) and the 3 x 3 maximum is read from there: 1.16 bicubic evaluations per
//                     pixel instead of nine.
//   segment painter   csrc/paint.h (the pose painter's tiles and lists) over primitives capsule, start disc, end disc per segment.
//   compactions       one 256-thread workgroup per image walks the rows (limbs) / grid points (offsets) in rounds of 256 and appends
//                     the kept ones in order (paint.h: ordered_slot); the running count stays in a register, n_segs[n] is written
//                     at the end.  A handful of workgroups: these run once per inspected batch over a few thousand candidates.
// Every arithmetic operation is one correctly rounded fp32 operation in the order written in the header: no contraction in this file
// (the fused multiply-adds of the two resamplers are explicit).
#pragma clang fp contract(off)

#include <limits.h>

#include "bicubic.h"
#include "paint.h"

namespace {

using namespace og_paint;

constexpr int HM_TILE_W = 64, HM_TILE_H = 16, HM_ROWS = HM_TILE_H * HM_TILE_W / THREADS;   // rows of pixels per thread
constexpr int HM_LDS_W = HM_TILE_W + 2, HM_LDS_H = HM_TILE_H + 2;

template <bool NMS>
__global__ void __launch_bounds__(THREADS)
draw_heatmap_kernel(unsigned char *__restrict__ images, const float *__restrict__ hm, const unsigned char *__restrict__ lut, int n_colors,
                    int C, int h, int w, int channel, float vmin, float range, float alpha)
{
    __shared__ float s_v[NMS ? HM_LDS_H : 1][NMS ? HM_LDS_W : 1];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int H = 4 * h, W = 4 * w;
    const int tx0 = blockIdx.x * HM_TILE_W, ty0 = blockIdx.y * HM_TILE_H;
    const float *plane = hm + ((size_t)n * C + channel) * h * w;
    if (NMS) {
        for (int i = tid; i < HM_LDS_H * HM_LDS_W; i += THREADS) {
            const int ly = i / HM_LDS_W, lx = i - ly * HM_LDS_W;
            const int Y = ty0 + ly - 1, X = tx0 + lx - 1;
            s_v[ly][lx] = (Y >= 0 && Y < H && X >= 0 && X < W) ? og_bicubic4_at(plane, h, w, Y, X) : 0.f;
        }
        __syncthreads();
    }
    const int lx = tid & (HM_TILE_W - 1), X = tx0 + lx;
    if (X >= W) return;
    const float top = (float)(n_colors - 1);
#pragma unroll
    for (int k = 0; k < HM_ROWS; ++k) {
        const int ly = (tid / HM_TILE_W) + k * (THREADS / HM_TILE_W), Y = ty0 + ly;
        if (Y >= H) break;
        float u;
        if (NMS) {
            const float v = s_v[ly + 1][lx + 1];
            float m = -INFINITY;                           // a NaN is never the larger one
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float t = s_v[ly + dy][lx + dx];
                    m = t > m ? t : m;
                }
            u = v * (m == v ? 1.f : 0.f);
        } else {
            u = og_bicubic4_at(plane, h, w, Y, X);
        }
        if (u != u) continue;
        const float t = fminf(fmaxf((u - vmin) / range, 0.f), 1.f);
        const int idx = (int)floorf(t * top + 0.5f);
        const unsigned char *col = lut + 3 * idx;
        unsigned char *pix = images + (((size_t)n * H + Y) * W + X) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float c = (float)pix[ch];
            c = c + ((float)col[ch] - c) * alpha;
            pix[ch] = (unsigned char)(int)floorf(c + 0.5f);
        }
    }
}

__global__ void __launch_bounds__(THREADS)
draw_segments_kernel(unsigned char *__restrict__ images, const float *__restrict__ segs, const int *__restrict__ n_segs, int H, int W,
                     int S, uint32_t line_rgb, uint32_t marker_rgb, float r_line, float r_start, float r_end, float alpha)
{
    const int n = blockIdx.z;
    const int count = min(max(n_segs[n], 0), S);         // a count beyond the table is clamped, never followed
    const float *img_segs = segs + (size_t)n * S * 4;
    paint_tile(images, H, W, 3 * count, alpha, [&](int idx, Entry &e) {   // (3 S < 2^30: checked by the host)
        const int s = idx / 3, j = idx - 3 * s;
        if ((j == 1 && !(r_start > 0.f)) || (j == 2 && !(r_end > 0.f))) return false;
        const float4 q = *reinterpret_cast<const float4 *>(img_segs + 4 * (size_t)s);
        if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(q.w))) return false;
        if (j == 0) e = make_entry(q.x, q.y, q.z, q.w, r_line, line_rgb);
        else if (j == 1) e = make_entry(q.x, q.y, q.x, q.y, r_start, marker_rgb);
        else e = make_entry(q.z, q.w, q.z, q.w, r_end, marker_rgb);
        return true;
    });
}

// Appends the rows `row(i, out4)` says to keep, i = 0 .. total-1 in order, to segs_n; returns nothing, writes *count_out.
template <class Row>
__device__ __forceinline__ void compact_rows(int total, float *__restrict__ segs_n, int *__restrict__ count_out, Row row)
{
    __shared__ int s_wave[WAVES];
    int count = 0;
    for (int base = 0; base < total; base += THREADS) {
        const int i = base + threadIdx.x;
        float4 o;
        const bool keep = i < total && row(i, o);
        int kept;
        const int slot = ordered_slot(keep, s_wave, kept);
        if (keep) *reinterpret_cast<float4 *>(segs_n + 4 * (size_t)(count + slot)) = o;   // count + slot <= i: inside the table
        count += kept;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count_out = count;
}

__global__ void __launch_bounds__(THREADS)
limbs_to_segments_kernel(const float *__restrict__ limbs, int L, int K, int limb, float dist_max, float *__restrict__ segs,
                         int *__restrict__ n_segs)
{
    const int n = blockIdx.x, total = L * K;
    const float *rows = limbs + (size_t)n * total * 13;
    compact_rows(total, segs + (size_t)n * total * 4, n_segs + n, [&](int i, float4 &o) {
        const float *r = rows + (size_t)i * 13;
        o = make_float4(r[0], r[1], r[3], r[4]);
        return (limb < 0 || i / K == limb) && o.x > 0.f && o.z > 0.f && r[8] <= dist_max;
    });
}

// one element of og_upsample_bilinear4_f32's output (upsample.hip: the same coordinates and fma chain)
__device__ __forceinline__ void lin_coord(int dpos, int n, int &i0, int &i1, float &l0, float &l1)
{
    float s = 0.25f * ((float)dpos + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i1 = (i0 + 1 < n) ? i0 + 1 : n - 1;
    l1 = s - (float)i0;
    l0 = 1.f - l1;
}

__device__ __forceinline__ float bilinear4_at(const float *__restrict__ p, int h, int w, int Y, int X)
{
    int x0, x1, y0, y1;
    float lx0, lx1, ly0, ly1;
    lin_coord(X, w, x0, x1, lx0, lx1);
    lin_coord(Y, h, y0, y1, ly0, ly1);
    const float a = __builtin_fmaf(p[(size_t)y0 * w + x0], lx0, p[(size_t)y0 * w + x1] * lx1);
    const float b = __builtin_fmaf(p[(size_t)y1 * w + x0], lx0, p[(size_t)y1 * w + x1] * lx1);
    return __builtin_fmaf(a, ly0, b * ly1);
}

__global__ void __launch_bounds__(THREADS)
offsets_to_segments_kernel(const float *__restrict__ hm, const float *__restrict__ off, int C, int L, int h, int w, int joint_from,
                           int limb, int step, float thre, int gw, int total, float *__restrict__ segs, int *__restrict__ n_segs)
{
    const int n = blockIdx.x;
    const float *heat = hm + ((size_t)n * C + joint_from) * h * w;
    const float *pu = off + ((size_t)n * 2 * L + 2 * limb) * h * w, *pv = pu + (size_t)h * w;
    compact_rows(total, segs + (size_t)n * total * 4, n_segs + n, [&](int i, float4 &o) {
        const int gy = i / gw, Y = gy * step, X = (i - gy * gw) * step;     // < 4h, 4w by the definition of the grid
        if (!(og_bicubic4_at(heat, h, w, Y, X) >= thre)) return false;
        const float U = bilinear4_at(pu, h, w, Y, X), V = bilinear4_at(pv, h, w, Y, X);
        const float fx = (float)X, fy = (float)Y;
        o = make_float4(fx, fy, fx + U, fy + V);
        return isfinite(U) && isfinite(V);
    });
}

inline bool finite_f(float v) { return v - v == 0.f; }

}  // namespace

OG_API long og_offsets_segments_capacity(int h, int w, int step)
{
    if (h <= 0 || w <= 0 || step <= 0 || h > INT_MAX / 4 || w > INT_MAX / 4) return 0;
    return (4l * h + step - 1) / step * ((4l * w + step - 1) / step);
}

OG_API int og_draw_heatmap_u8(void *images, const float *hm, const unsigned char *lut, int n_colors, int N, int C, int h, int w,
                              int channel, float vmin, float vmax, float alpha, int nms, void *stream)
{
    const char *name = "og_draw_heatmap_u8";
    OG_REQUIRE(images && hm && lut, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && h > 0 && w > 0 && h <= INT_MAX / 4 && w <= INT_MAX / 4, OG_EINVAL,
               "%s: bad shape (N %d, C %d, h %d, w %d)", name, N, C, h, w);
    OG_REQUIRE(channel >= 0 && channel < C, OG_EINVAL, "%s: channel %d outside [0, %d)", name, channel, C);
    OG_REQUIRE(n_colors > 0, OG_EINVAL, "%s: n_colors %d (the table needs at least one colour)", name, n_colors);
    OG_REQUIRE(finite_f(vmin) && finite_f(vmax) && vmax > vmin, OG_EINVAL, "%s: vmin %g / vmax %g (finite, vmin < vmax)", name,
               (double)vmin, (double)vmax);
    OG_REQUIRE(alpha > 0.f && alpha <= 1.f, OG_EINVAL, "%s: alpha %g outside (0, 1]", name, (double)alpha);
    const long gx = (4l * w + HM_TILE_W - 1) / HM_TILE_W, gy = (4l * h + HM_TILE_H - 1) / HM_TILE_H;
    OG_REQUIRE(N <= 65535 && gy <= 65535, OG_EINVAL, "%s: grid too large (N %d, h %d)", name, N, h);
    auto kernel = nms ? draw_heatmap_kernel<true> : draw_heatmap_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)N), dim3(THREADS), 0, (hipStream_t)stream,
                       static_cast<unsigned char *>(images), hm, lut, n_colors, C, h, w, channel, vmin, vmax - vmin, alpha);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_draw_segments_u8(void *images, const float *segs, const int *n_segs, int N, int H, int W, int S, unsigned int line_rgb,
                               unsigned int marker_rgb, float line_width, float r_start, float r_end, float alpha, void *stream)
{
    const char *name = "og_draw_segments_u8";
    OG_REQUIRE(images && segs && n_segs, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && H > 0 && W > 0 && S > 0, OG_EINVAL, "%s: bad shape (N %d, H %d, W %d, S %d)", name, N, H, W, S);
    OG_REQUIRE(alpha > 0.f && alpha <= 1.f, OG_EINVAL, "%s: alpha %g outside (0, 1]", name, (double)alpha);
    OG_REQUIRE(line_width >= 0.f && line_width <= 1e6f && r_start >= 0.f && r_start <= 1e6f && r_end >= 0.f && r_end <= 1e6f, OG_EINVAL,
               "%s: line_width %g / r_start %g / r_end %g (finite, >= 0)", name, (double)line_width, (double)r_start, (double)r_end);
    OG_REQUIRE((uintptr_t)segs % 16 == 0, OG_EINVAL, "%s: segs must be 16-byte aligned", name);
    OG_REQUIRE(3l * S < (1l << 30), OG_EINVAL, "%s: S %d too large", name, S);
    const long gx = ((long)W + TILE_W - 1) / TILE_W, gy = ((long)H + TILE_H - 1) / TILE_H;
    OG_REQUIRE(N <= 65535 && gy <= 65535, OG_EINVAL, "%s: grid too large (N %d, H %d)", name, N, H);
    hipLaunchKernelGGL(draw_segments_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)N), dim3(THREADS), 0, (hipStream_t)stream,
                       static_cast<unsigned char *>(images), segs, n_segs, H, W, S, line_rgb & 0xffffffu, marker_rgb & 0xffffffu,
                       line_width / 2.f, r_start, r_end, alpha);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_limbs_to_segments_f32(const float *limbs, int N, int L, int K, int limb, float dist_max, float *segs, int *n_segs,
                                    void *stream)
{
    const char *name = "og_limbs_to_segments_f32";
    OG_REQUIRE(limbs && segs && n_segs, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && L > 0 && K > 0 && (long)L * K < (1l << 28), OG_EINVAL, "%s: bad shape (N %d, L %d, K %d)", name, N, L, K);
    OG_REQUIRE(limb < L, OG_EINVAL, "%s: limb %d outside [0, %d) (negative: every limb type)", name, limb, L);
    OG_REQUIRE((uintptr_t)segs % 16 == 0, OG_EINVAL, "%s: segs must be 16-byte aligned", name);
    hipLaunchKernelGGL(limbs_to_segments_kernel, dim3((unsigned)N), dim3(THREADS), 0, (hipStream_t)stream, limbs, L, K, limb, dist_max,
                       segs, n_segs);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_offsets_to_segments_f32(const float *hm, const float *off, int N, int C, int L, int h, int w, int joint_from, int limb,
                                      int step, float thre, float *segs, int *n_segs, void *stream)
{
    const char *name = "og_offsets_to_segments_f32";
    OG_REQUIRE(hm && off && segs && n_segs, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && L > 0 && h > 0 && w > 0 && h <= (1 << 22) && w <= (1 << 22), OG_EINVAL,
               "%s: bad shape (N %d, C %d, L %d, h %d, w %d)", name, N, C, L, h, w);
    OG_REQUIRE(joint_from >= 0 && joint_from < C, OG_EINVAL, "%s: joint_from %d outside [0, %d)", name, joint_from, C);
    OG_REQUIRE(limb >= 0 && limb < L, OG_EINVAL, "%s: limb %d outside [0, %d)", name, limb, L);
    OG_REQUIRE(step > 0, OG_EINVAL, "%s: step %d (> 0)", name, step);
    OG_REQUIRE((uintptr_t)segs % 16 == 0, OG_EINVAL, "%s: segs must be 16-byte aligned", name);
    const long total = og_offsets_segments_capacity(h, w, step);
    OG_REQUIRE(total < (1l << 28), OG_EINVAL, "%s: %ld grid points (h %d, w %d, step %d): too many", name, total, h, w, step);
    hipLaunchKernelGGL(offsets_to_segments_kernel, dim3((unsigned)N), dim3(THREADS), 0, (hipStream_t)stream, hm, off, C, L, h, w,
                       joint_from, limb, step, thre, (int)((4l * w + step - 1) / step), (int)total, segs, n_segs);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
