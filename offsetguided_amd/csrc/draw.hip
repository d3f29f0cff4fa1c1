// Pose painter: skeleton capsules and keypoint discs blended over a uint8 RGB batch in place (visualization/__init__.py:draw_poses,
// evaluate.py --show-detected-poses; the semantics are spelled out at og_draw_poses_u8 in include/og_decoder.h).
//
// The tile / list machinery (32 x 8 pixel tiles, the image's primitive list culled and compacted in rounds of 256 into an LDS list,
// blended in primitive order) is csrc/paint.h, shared with the segment painter of views.hip; this file supplies the primitives:
// person-major, the L limbs, then the K keypoints.
// Every arithmetic operation is one correctly rounded fp32 operation in the order written in the header: no contraction in this file.
#pragma clang fp contract(off)

#include "paint.h"

namespace {

using namespace og_paint;

__global__ void __launch_bounds__(THREADS)
draw_poses_kernel(unsigned char *__restrict__ images, const float *__restrict__ poses, const int *__restrict__ n_persons,
                  const int *__restrict__ skeleton, const unsigned char *__restrict__ palette, int n_colors, int H, int W, int P, int K,
                  int L, float r_line, float r_mark, float alpha)
{
    const int n = blockIdx.z;
    const int persons = min(max(n_persons[n], 0), P);    // a count beyond the table is clamped, never followed
    const int per = L + K;                               // (P * (L + K) < 2^30: checked by the host)
    const float *img_poses = poses + (size_t)n * P * K * 3;
    paint_tile(images, H, W, persons * per, alpha, [&](int idx, Entry &e) {
        const int p = idx / per, j = idx - p * per;
        const float *person = img_poses + (size_t)p * K * 3;
        const int a = j < L ? skeleton[2 * j] : j - L, b = j < L ? skeleton[2 * j + 1] : j - L;
        if (a < 0 || a >= K || b < 0 || b >= K) return false;   // (the Python wrapper refuses such a skeleton; never read beyond the table)
        const float ax = person[3 * a], ay = person[3 * a + 1], av = person[3 * a + 2];
        const float bx = person[3 * b], by = person[3 * b + 1], bv = person[3 * b + 2];
        if (!(av > 0.f && bv > 0.f && isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by))) return false;
        const unsigned char *col = palette + 3 * (p % n_colors);
        e = make_entry(ax, ay, bx, by, j < L ? r_line : r_mark, (uint32_t)col[0] | (uint32_t)col[1] << 8 | (uint32_t)col[2] << 16);
        return true;
    });
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
