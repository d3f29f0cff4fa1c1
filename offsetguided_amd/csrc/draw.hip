// Pose painter: skeleton capsules and keypoint discs blended over a uint8 RGB batch in place (visualization/__init__.py:draw_poses,
// evaluate.py --show-detected-poses; the semantics are spelled out at og_draw_poses_u8 in include/og_decoder.h).
//
// One 256-thread workgroup per tile of 32 x 8 pixels (a tile row = 96 contiguous bytes), image = blockIdx.z, one pixel per thread.
// The image's primitive list (person-major: the L limbs, then the K keypoints) is walked in rounds of 256, one primitive per thread:
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
// Every arithmetic operation is one correctly rounded fp32 operation in the order written in the header: no contraction in this file.
#include <math.h>

#include "og_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE_W = 32, TILE_H = 8, THREADS = TILE_W * TILE_H, WAVES = THREADS / 64;
constexpr int LIST_CAP = 512;   // entries; a batch is blended as soon as fewer than THREADS slots are free

// ax, ay, dx, dy | 1-or-len2, r, colour (r | g << 8 | b << 16), unused.  A disc is a segment with dx = dy = 0.
struct Entry {
    float4 seg, aux;
};
static_assert(sizeof(Entry) == 32, "two 16-byte LDS reads per entry");

__global__ void __launch_bounds__(THREADS)
draw_poses_kernel(unsigned char *__restrict__ images, const float *__restrict__ poses, const int *__restrict__ n_persons,
                  const int *__restrict__ skeleton, const unsigned char *__restrict__ palette, int n_colors, int H, int W, int P, int K,
                  int L, float r_line, float r_mark, float alpha)
{
    __shared__ __attribute__((aligned(16))) Entry s_list[LIST_CAP];
    __shared__ int s_wave[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.z;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const int ix = tx0 + (tid & (TILE_W - 1)), iy = ty0 + tid / TILE_W;
    const bool inside = ix < W && iy < H;
    const float px = (float)ix, py = (float)iy;
    const float tile_x0 = (float)tx0, tile_x1 = (float)(tx0 + TILE_W - 1), tile_y0 = (float)ty0, tile_y1 = (float)(ty0 + TILE_H - 1);
    const int persons = min(max(n_persons[n], 0), P);    // a count beyond the table is clamped, never followed
    const int per = L + K, M = persons * per;            // (P * (L + K) < 2^30: checked by the host)
    const float *img_poses = poses + (size_t)n * P * K * 3;
    unsigned char *pix = images + (((size_t)n * H + iy) * W + ix) * 3;

    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    bool loaded = false, touched = false;
    int count = 0;                                       // entries in s_list (uniform over the workgroup)
    for (int base = 0; base < M; base += THREADS) {
        // ---- cull: primitive base + tid
        const int idx = base + tid;
        bool pass = false;
        Entry e{};
        if (idx < M) {
            const int p = idx / per, j = idx - p * per;
            const float *person = img_poses + (size_t)p * K * 3;
            int a, b;
            if (j < L) {
                a = skeleton[2 * j];
                b = skeleton[2 * j + 1];
                e.aux.y = r_line;
            } else {
                a = b = j - L;
                e.aux.y = r_mark;
            }
            if (a >= 0 && a < K && b >= 0 && b < K) {    // (the Python wrapper refuses such a skeleton; never read beyond the table)
                const float ax = person[3 * a], ay = person[3 * a + 1], av = person[3 * a + 2];
                const float bx = person[3 * b], by = person[3 * b + 1], bv = person[3 * b + 2];
                if (av > 0.f && bv > 0.f && isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by)) {
                    const float dx = bx - ax, dy = by - ay;
                    const float len2 = dx * dx + dy * dy;
                    const float grow = e.aux.y + 1.5f;
                    pass = fmaxf(ax, bx) + grow >= tile_x0 && fminf(ax, bx) - grow <= tile_x1 &&
                           fmaxf(ay, by) + grow >= tile_y0 && fminf(ay, by) - grow <= tile_y1;
                    const unsigned char *col = palette + 3 * (p % n_colors);
                    e.seg = make_float4(ax, ay, dx, dy);
                    e.aux.x = len2 == 0.f ? 1.f : len2;  // t = 0 / 1 = 0 on a zero-length limb and on a disc
                    e.aux.z = __builtin_bit_cast(float, (uint32_t)col[0] | (uint32_t)col[1] << 8 | (uint32_t)col[2] << 16);
                }
            }
        }
        // ---- ordered compaction into the list
        const unsigned long long m = __ballot(pass);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (pass) s_list[count + before + __popcll(m & ((1ull << lane) - 1ull))] = e;   // < count + THREADS <= LIST_CAP
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

}  // namespace

OG_API int og_draw_poses_u8(void *images, const float *poses, const int *n_persons, const int *skeleton, const unsigned char *palette,
                            int n_colors, int N, int H, int W, int P, int K, int L, float line_width, float marker_radius, float alpha,
                            void *stream)
{
    const char *name = "og_draw_poses_u8";
    OG_REQUIRE(images && poses && n_persons && skeleton && palette, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && H > 0 && W > 0 && P > 0 && K > 0 && L > 0, OG_EINVAL, "%s: bad shape (N %d, H %d, W %d, P %d, K %d, L %d)", name,
               N, H, W, P, K, L);
    OG_REQUIRE(n_colors > 0, OG_EINVAL, "%s: n_colors %d (the palette needs at least one colour)", name, n_colors);
    OG_REQUIRE(alpha > 0.f && alpha <= 1.f, OG_EINVAL, "%s: alpha %g outside (0, 1]", name, (double)alpha);
    OG_REQUIRE(line_width >= 0.f && line_width <= 1e6f && marker_radius >= 0.f && marker_radius <= 1e6f, OG_EINVAL,
               "%s: line_width %g / marker_radius %g (finite, >= 0)", name, (double)line_width, (double)marker_radius);
    OG_REQUIRE((long)P * ((long)L + K) < (1L << 30), OG_EINVAL, "%s: P * (L + K) too large", name);
    const long gx = ((long)W + TILE_W - 1) / TILE_W, gy = ((long)H + TILE_H - 1) / TILE_H;
    OG_REQUIRE(N <= 65535 && gy <= 65535, OG_EINVAL, "%s: grid too large (N %d, H %d)", name, N, H);
    hipLaunchKernelGGL(draw_poses_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)N), dim3(THREADS), 0, (hipStream_t)stream,
                       static_cast<unsigned char *>(images), poses, n_persons, skeleton, palette, n_colors, H, W, P, K, L,
                       line_width / 2.f, marker_radius, alpha);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
