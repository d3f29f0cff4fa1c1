// hmp_NMS with a window other than the decoder's 3 (reference decoder/heatmap.py:15-35): heat * (maxpool_k(heat) == heat),
// zero padding, odd k up to 7.  The three device ops of the reference (pad, max_pool2d, multiply) as one kernel.
//
// A workgroup owns a 64 x 16 tile of one plane: the tile and its halo of (k-1)/2 cells (zeros outside the plane: the padding takes
// part in the maximum, as it does in the padded pool) are staged in LDS, the window maximum is taken separably (along the rows,
// then down the columns), and every element is written as heat * 1 or heat * 0 -- the product itself, so a suppressed element
// keeps the sign of its input and a non-finite one gives what the reference's multiply gives.  Compares are exact; a NaN in the
// window makes the maximum NaN (max_pool2d's rule), which equals nothing.
#include "og_common.h"

namespace {

constexpr int kTileW = 64, kTileH = 16, kMaxPad = 3;
constexpr int kLdsW = kTileW + 2 * kMaxPad, kLdsH = kTileH + 2 * kMaxPad;

__device__ __forceinline__ float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(256)
nms_window_kernel(const float *__restrict__ heat, float *__restrict__ out, int H, int W, int pad, int tiles_x, int tiles_y)
{
    __shared__ float s_in[kLdsH][kLdsW];
    __shared__ float s_row[kLdsH][kTileW];
    const int tile = blockIdx.x % (tiles_x * tiles_y);
    const size_t plane = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const float *src = heat + plane * (size_t)H * W;
    float *dst = out + plane * (size_t)H * W;
    const int lw = kTileW + 2 * pad, lh = kTileH + 2 * pad;
    for (int i = threadIdx.x; i < lw * lh; i += blockDim.x) {
        const int ly = i / lw, lx = i % lw;
        const int y = y0 + ly - pad, x = x0 + lx - pad;
        s_in[ly][lx] = (y >= 0 && y < H && x >= 0 && x < W) ? src[(size_t)y * W + x] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < lh * kTileW; i += blockDim.x) {
        const int ly = i / kTileW, lx = i % kTileW;
        float m = s_in[ly][lx];
        for (int d = 1; d <= 2 * pad; ++d) m = pool_max(m, s_in[ly][lx + d]);
        s_row[ly][lx] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTileH * kTileW; i += blockDim.x) {
        const int ly = i / kTileW, lx = i % kTileW;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        float m = s_row[ly][lx];
        for (int d = 1; d <= 2 * pad; ++d) m = pool_max(m, s_row[ly + d][lx]);
        const float v = s_in[ly + pad][lx + pad];
        dst[(size_t)y * W + x] = v * (m == v ? 1.f : 0.f);
    }
}

}  // namespace

OG_API int og_hmp_nms_k_f32(const float *heat, long planes, int H, int W, int kernel, float *out, void *stream)
{
    const char *name = "og_hmp_nms_k_f32";
    OG_REQUIRE(heat && out, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(planes > 0 && H > 0 && W > 0, OG_EINVAL, "%s: bad shape", name);
    OG_REQUIRE(kernel >= 1 && kernel <= 2 * kMaxPad + 1 && kernel % 2 == 1, OG_EUNSUPPORTED, "%s: window must be odd, 1..%d (got %d)",
               name, 2 * kMaxPad + 1, kernel);
    const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
    const long blocks = planes * tiles_x * tiles_y;
    OG_REQUIRE(blocks < (1l << 31), OG_EINVAL, "%s: too many tiles", name);
    hipLaunchKernelGGL(nms_window_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, heat, out, H, W, (kernel - 1) / 2,
                       tiles_x, tiles_y);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
