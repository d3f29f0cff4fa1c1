// The tile / list machinery of the capsule-and-disc painters (og_draw_poses_u8 in draw.hip, og_draw_segments_u8 in views.hip; the
// semantics are spelled out at og_draw_poses_u8 in include/og_decoder.h).
//
// One 256-thread workgroup per tile of 32 x 8 pixels (a tile row = 96 contiguous bytes), image = blockIdx.z, one pixel per thread.
// The image's M primitives are walked in rounds of 256, one primitive per thread; `gen(idx, e)` says whether primitive idx is drawn
// and fills its entry (end point a, b - a, radius, colour):
//   cull   a primitive passes when its bounding box grown by r + 1.5 meets the tile.  A pixel is covered only within r + 0.5 of the
//          primitive, which lies inside its box: the extra pixel is slack for the rounding of the box arithmetic, so culling never
//          changes a result.  Passing primitives are compacted IN PRIMITIVE ORDER into an LDS list: __ballot per wave, the waves'
//          counts prefix-summed in wave order (wave w holds primitives 64 w ... 64 w + 63 of the round), popcount of the lower lanes.
//   blend  when the list cannot take another full round (or the walk is over) every thread loops over it: all lanes read the same
//          32-byte entry (two broadcast ds_read_b128), the pixel's three channels stay in fp32 registers across batches, so a tile
//          under any number of primitives is served in batches of at most LIST_CAP with nothing dropped and the order kept.
// A tile whose list stays empty never touches the image; a pixel is loaded at the tile's first non-empty batch and stored once, at the
// end, only if some primitive covered it.
// LDS: 16 KiB + 16 B per workgroup -- the 8 workgroups (32 waves) a CU can hold fit its 160 KiB, so LDS never limits residency.
// Every arithmetic operation is one correctly rounded fp32 operation in the order written in the header: the including file turns
// contraction off (#pragma clang fp contract(off)) before it includes this one.
#pragma once
#include <math.h>

#include "og_common.h"

namespace og_paint {

constexpr int TILE_W = 32, TILE_H = 8, THREADS = TILE_W * TILE_H, WAVES = THREADS / 64;
constexpr int LIST_CAP = 512;   // entries; a batch is blended as soon as fewer than THREADS slots are free

// ax, ay, dx, dy | 1-or-len2, r, colour (r | g << 8 | b << 16), unused.  A disc is a segment with dx = dy = 0.
struct Entry {
    float4 seg, aux;
};
static_assert(sizeof(Entry) == 32, "two 16-byte LDS reads per entry");

// the entry of the capsule a -> b (a disc: b = a) of radius r; all four coordinates finite
__device__ __forceinline__ Entry make_entry(float ax, float ay, float bx, float by, float r, uint32_t rgb)
{
    const float dx = bx - ax, dy = by - ay;
    const float len2 = dx * dx + dy * dy;
    Entry e;
    e.seg = make_float4(ax, ay, dx, dy);
    e.aux = make_float4(len2 == 0.f ? 1.f : len2,   // t = 0 / 1 = 0 on a zero-length limb and on a disc
                        r, __builtin_bit_cast(float, rgb), 0.f);
    return e;
}

// Position of `pass` among the passing threads of the workgroup in thread order, and their number (uniform).  One barrier inside; the
// caller puts another between two calls (s_wave is rewritten).
__device__ __forceinline__ int ordered_slot(bool pass, int *s_wave, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(pass);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int c = s_wave[w];
        before += w < wave ? c : 0;
        total += c;
    }
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// Paints the M primitives of image blockIdx.z over the workgroup's tile of images (N, H, W, 3).
template <class Gen>
__device__ __forceinline__ void paint_tile(unsigned char *__restrict__ images, int H, int W, int M, float alpha, Gen gen)
{
    __shared__ __attribute__((aligned(16))) Entry s_list[LIST_CAP];
    __shared__ int s_wave[WAVES];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const int ix = tx0 + (tid & (TILE_W - 1)), iy = ty0 + tid / TILE_W;
    const bool inside = ix < W && iy < H;
    const float px = (float)ix, py = (float)iy;
    const float tile_x0 = (float)tx0, tile_x1 = (float)(tx0 + TILE_W - 1), tile_y0 = (float)ty0, tile_y1 = (float)(ty0 + TILE_H - 1);
    unsigned char *pix = images + (((size_t)n * H + iy) * W + ix) * 3;

    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    bool loaded = false, touched = false;
    int count = 0;                                       // entries in s_list (uniform over the workgroup)
    for (int base = 0; base < M; base += THREADS) {
        // ---- cull: primitive base + tid
        const int idx = base + tid;
        bool pass = false;
        Entry e{};
        if (idx < M && gen(idx, e)) {
            const float ax = e.seg.x, ay = e.seg.y, bx = ax + e.seg.z, by = ay + e.seg.w;   // (within an ulp of b: the slack covers it)
            const float grow = e.aux.y + 1.5f;
            pass = fmaxf(ax, bx) + grow >= tile_x0 && fminf(ax, bx) - grow <= tile_x1 &&
                   fmaxf(ay, by) + grow >= tile_y0 && fminf(ay, by) - grow <= tile_y1;
        }
        // ---- ordered compaction into the list
        int total;
        const int slot = ordered_slot(pass, s_wave, total);
        if (pass) s_list[count + slot] = e;              // < count + THREADS <= LIST_CAP
        count += total;
        __syncthreads();
        // ---- blend a batch: the list could not take another round, or this was the last one
        if (count + THREADS > LIST_CAP || base + THREADS >= M) {
            if (count > 0 && inside) {
                if (!loaded) {
                    c0 = (float)pix[0];
                    c1 = (float)pix[1];
                    c2 = (float)pix[2];
                    loaded = true;
                }
                for (int i = 0; i < count; ++i) {
                    const float4 s = s_list[i].seg;
                    const float4 q = s_list[i].aux;
                    const float ex = px - s.x, ey = py - s.y;
                    float t = (ex * s.z + ey * s.w) / q.x;
                    t = fminf(fmaxf(t, 0.f), 1.f);
                    const float qx = s.x + t * s.z, qy = s.y + t * s.w;
                    const float fx = px - qx, fy = py - qy;
                    const float d = sqrtf(fx * fx + fy * fy);
                    const float cov = fminf(fmaxf(q.y + 0.5f - d, 0.f), 1.f);
                    if (cov > 0.f) {
                        const uint32_t rgb = __builtin_bit_cast(uint32_t, q.z);
                        const float wgt = cov * alpha;
                        c0 = c0 + ((float)(rgb & 255u) - c0) * wgt;
                        c1 = c1 + ((float)(rgb >> 8 & 255u) - c1) * wgt;
                        c2 = c2 + ((float)(rgb >> 16 & 255u) - c2) * wgt;
                        touched = true;
                    }
                }
            }
            count = 0;
            __syncthreads();                             // the next round overwrites the list
        }
    }
    if (touched) {
        pix[0] = (unsigned char)(int)floorf(c0 + 0.5f);
        pix[1] = (unsigned char)(int)floorf(c1 + 0.5f);
        pix[2] = (unsigned char)(int)floorf(c2 + 0.5f);
    }
}

}  // namespace og_paint
