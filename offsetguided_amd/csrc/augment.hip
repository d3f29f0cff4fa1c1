// Training augmentation on the device: the step WarpAffineTransforms does on the host in the reference (transforms/affine.py:71-278:
// cv2.warpAffine of the image and of mask_miss, the same matrix on the keypoints, then ToTensor + Normalize) for a batch of raw
// uint8 images already in HBM, as ONE launch per batch that writes the fp32 NCHW network input.
//
// The warp is a SPECIFICATION OF THIS LIBRARY'S OWN in integer arithmetic (a 4-tap cubic with 32 sub-pixel phases and 2^11
// fixed-point taps: the shape of OpenCV's 8-bit remap, not a claim about its bits -- cv2 is absent from the build, parity with
// cv2.warpAffine(INTER_CUBIC) is UNPINNED).  It is held bit for bit to the numpy restatement tests/augment_common.py.
//
// One warped value.  D = [a b c; d e f] (float64) = the first two rows of inv(M), the destination -> source map; S = the side of
// the destination square; src (h, w, C) uint8; border[C] the colour outside.  For destination pixel (x, y), channel ch:
//   1. X = rint((a * x) * 1024) + rint(((b * y) + c) * 1024) + 16      int32 sum of two float64 values rounded to nearest even;
//      every float64 product and sum is rounded on its own (no fused multiply-add); Y likewise with d, e, f.
//      X >>= 5 (arithmetic);  sx = X >> 5,  px = X & 31;  Y >>= 5;  sy = Y >> 5,  py = Y & 31           (32 phases per axis)
//   2. taps of phase p: x = p / 32 in fp32 and, every operation one fp32 operation, left to right, A = -0.75,
//        c0 = ((A*(x+1) - 5*A)*(x+1) + 8*A)*(x+1) - 4*A,  c1 = ((A+2)*x - (A+3))*x*x + 1,
//        c2 = ((A+2)*(1-x) - (A+3))*(1-x)*(1-x) + 1,      c3 = 1 - c0 - c1 - c2               (cubic_taps of preprocess.hip)
//        t[k] = rint(c[k] * 2048) (to nearest even); then 2048 - (t0+t1+t2+t3), which is -1, 0 or +1, is added to the LARGEST tap
//        (the first one among equals), so that every phase sums to 2048.  Phase 0 is (0, 2048, 0, 0).
//   3. v = clamp((sum_j sum_i s(sy-1+j, sx-1+i, ch) * wx[i] * wy[j] + 2^21) >> 22, 0, 255) in int32, wx = taps(px), wy = taps(py),
//      s(r, q, ch) = src[r][q][ch] if 0 <= r < h and 0 <= q < w, else border[ch].
//      No overflow: the largest sum of |t[k]| over the 32 phases is 2816 (phases 15..17: 203 + 1299 + 1131 + 179 and
//      192 + 1216 + 1216 + 192), so every partial sum is at most 255 * 2816 * 2816 = 2 022 113 280 in magnitude, and with the
//      rounding term 2 024 210 432 < 2^31 = 2 147 483 648.  Integer sums are exact, so their grouping is free: the kernel sums a
//      row first.  A window that lies wholly outside the image gives border[ch] exactly (the taps sum to 2^22), without the sums.
//   4. every source read is predicated: a tap outside the image never forms an address.
// The callers guarantee |a|*S + |b|*S + |c| < 2^20 (and the same for d, e, f; checked by the entry points), so X and Y fit int32.
// og_warp_affine_batch_u8 then stores (v / 255 - mean[ch]) / std[ch] in fp32 -- ToTensor + Normalize, the expression and operation
// order of preprocess.hip -- and, on request, v itself; og_warp_affine_mask_u8 stores v of single-channel planes.
//
// Shape: one workgroup per 64 x 16 destination tile of one image (blockIdx.y), a thread owns four consecutive x of one row: per-row
// terms once per thread, one 16-byte store per NCHW plane.  The taps are read as bytes through L1 (the 16 taps of neighbouring
// pixels overlap heavily); the source is not staged in LDS (under rotation and scale 0.5 a tile's footprint is large and irregular).
// LDS holds the 32 x 4 tap table only, computed by the workgroup's first 32 threads.
//
// og_warp_affine_photo_batch_u8 is the same kernel with the photometric epilogue of csrc/photometric.h (ColorTint, Gray; a descriptor
// per image, by value like the geometry) between v and the normalisation: v' = epilogue(v) is what gets normalised, out_u8 still
// receives v itself (the JPEG round trip of csrc/jpeg_sim.hip reads it).  That instantiation also builds the tint's two division
// tables (2 KiB) in LDS.  With every mode 0 it stores what og_warp_affine_batch_u8 stores.
//
// og_affine_joints_jitter_f32 adds AnnotationJitter (transforms/annotations.py:89-111) behind the keypoint transform: rows of persons
// in use of a gated image get x += eps * (((u - 0.5) + shift) * 2), y likewise, u the row's two fp32 noise values, every operation one
// fp32 operation in this order; after the visibility test, which is not repeated (the reference jitters after the warp and never culls).
#include <math.h>

#include <type_traits>

#include "og_common.h"
#include "photometric.h"

namespace {

constexpr int kWarpTW = 64, kWarpTH = 16, kWarpBatchMax = 32;

// geometry of up to kWarpBatchMax images, by value in the kernel arguments (no device-side descriptor upload)
struct WarpBatch {
    long off[kWarpBatchMax];          // byte offset of the image's pixels in the packed uint8 buffer
    int h[kWarpBatchMax], w[kWarpBatchMax];
    double D[kWarpBatchMax][6];
};

struct WarpArgs {
    float mean[3], stdv[3];
    int border[3];
};

// photometric descriptors of a launch's images; the plain instantiations carry an empty argument instead
struct PhotoBatch {
    photo::Desc d[kWarpBatchMax];
};
struct NoPhoto {};
template <bool PHOTO>
using PhotoArg = std::conditional_t<PHOTO, PhotoBatch, NoPhoto>;

// specification step 2
__device__ __forceinline__ void phase_taps(int p, short (&t)[4])
{
    const float x = (float)p / 32.f;
    const float A = -0.75f;
    float c[4];
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
    int v[4], sum = 0, big = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = __float2int_rn(c[k] * 2048.f);
        sum += v[k];
    }
#pragma unroll
    for (int k = 1; k < 4; ++k) big = v[k] > v[big] ? k : big;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = (short)(v[k] + (k == big ? 2048 - sum : 0));
}

// specification step 1 for one axis: rint((m0 * x) * 1024) + row + 16, row = rint(((m1 * y) + m2) * 1024)
__device__ __forceinline__ int warp_row_term(double m1, double m2, int y)
{
    return __double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m1, (double)y), m2), 1024.0));
}
__device__ __forceinline__ int warp_coord(double m0, int x, int row)
{
    return (__double2int_rn(__dmul_rn(__dmul_rn(m0, (double)x), 1024.0)) + row + 16) >> 5;
}

// C = channels per source pixel (3: images, 1: mask planes).  NORM: write the normalised fp32 NCHW tensor (and v as NHWC bytes if
// out_u8 is not null); otherwise v goes to out_u8 (N,S,S) planes.  vec4: S % 4 == 0 and the outputs are 16-byte (fp32) / 4-byte
// (planes) aligned, so a thread's four values leave in one store.  PHOTO: csrc/photometric.h between v and the normalisation.
template <int C, bool NORM, bool PHOTO = false>
__global__ void __launch_bounds__(256)
warp_affine_kernel(const unsigned char *__restrict__ raw, WarpBatch b, WarpArgs a, int S, int tiles_x, float *__restrict__ out_f,
                   unsigned char *__restrict__ out_u8, int vec4, PhotoArg<PHOTO> pb)
{
    static_assert(!PHOTO || (NORM && C == 3), "the photometric epilogue works on the RGB triple that gets normalised");
    __shared__ short taps[32][4];
    const int *sdiv = nullptr, *hdiv = nullptr;
    if constexpr (PHOTO) {
        __shared__ int divs[2][256];
        photo::build_tables(divs[0], divs[1], threadIdx.x);
        sdiv = divs[0];
        hdiv = divs[1];
    }
    if (threadIdx.x < 32) {
        short t[4];
        phase_taps(threadIdx.x, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) taps[threadIdx.x][k] = t[k];
    }
    __syncthreads();
    const int n = blockIdx.y;
    const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
    const int x0 = tile_x * kWarpTW + (threadIdx.x & 15) * 4, y = tile_y * kWarpTH + (threadIdx.x >> 4);
    if (x0 >= S || y >= S) return;
    const int h = b.h[n], w = b.w[n];
    const unsigned char *__restrict__ src = raw + b.off[n];
    const double m0 = b.D[n][0], m3 = b.D[n][3];
    const int rowX = warp_row_term(b.D[n][1], b.D[n][2], y), rowY = warp_row_term(b.D[n][4], b.D[n][5], y);
    int v[4][C];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = min(x0 + i, S - 1);                      // (a column beyond S repeats the last one: nobody stores it)
        const int X = warp_coord(m0, x, rowX), Y = warp_coord(m3, x, rowY);
        const int sx = X >> 5, px = X & 31, sy = Y >> 5, py = Y & 31;
        if (sx + 2 < 0 || sx - 1 >= w || sy + 2 < 0 || sy - 1 >= h) {
#pragma unroll
            for (int c = 0; c < C; ++c) v[i][c] = a.border[c];
            continue;
        }
        int wx[4], wy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { wx[k] = taps[px][k]; wy[k] = taps[py][k]; }
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = sy - 1 + j;
            const bool row_in = r >= 0 && r < h;
            int hs[C];
#pragma unroll
            for (int c = 0; c < C; ++c) hs[c] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = sx - 1 + k;
                const bool in = row_in && q >= 0 && q < w;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    int s = a.border[c];
                    if (in) s = src[((size_t)r * w + q) * C + c];
                    hs[c] += s * wx[k];
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += hs[c] * wy[j];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) v[i][c] = min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
    }
    const size_t px0 = ((size_t)n * S + y) * S + x0;           // pixel index of (n, y, x0) in an (N,S,S) plane
    if (NORM) {
        auto store_u8 = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < S) {
#pragma unroll
                    for (int c = 0; c < C; ++c) out_u8[(px0 + i) * C + c] = (unsigned char)v[i][c];
                }
        };
        if constexpr (PHOTO) {
            if (out_u8) store_u8();                            // v itself, before the epilogue
            const photo::Desc d = pb.d[n];
            if (d.mode) {
#pragma unroll
                for (int i = 0; i < 4; ++i) photo::apply(v[i][0], v[i][1], v[i][2], d, sdiv, hdiv);
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = ((float)v[i][c] / 255.f - a.mean[c]) / a.stdv[c];   // ToTensor, Normalize
            float *dst = out_f + ((size_t)n * C + c) * S * S + (size_t)y * S + x0;
            if (vec4) {
                *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x0 + i < S) dst[i] = o[i];
            }
        }
        if constexpr (!PHOTO) {
            if (out_u8) store_u8();
        }
    } else {
        if (vec4) {
            *reinterpret_cast<uchar4 *>(out_u8 + px0) =
                make_uchar4((unsigned char)v[0][0], (unsigned char)v[1][0], (unsigned char)v[2][0], (unsigned char)v[3][0]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < S) out_u8[px0 + i] = (unsigned char)v[i][0];
        }
    }
}

// ---- keypoints: _affine_keypoints, transforms/affine.py:192-227 ----
constexpr int kLrMax = 16;
struct JointBatch {
    double M[kWarpBatchMax][6], scale[kWarpBatchMax];
    int flip[kWarpBatchMax];
};
struct LrTable {
    int left[kLrMax], right[kLrMax], n;
};
struct JitterBatch {
    float eps[kWarpBatchMax], shift[kWarpBatchMax];
    int gate[kWarpBatchMax];
};

// one thread per keypoint row (n, p, k) of joints (N,P,K,4): rows [x, y, v, scale]; noise (N,P,K) pairs or null (no jitter at all)
__global__ void __launch_bounds__(256)
affine_joints_kernel(const float4 *__restrict__ joints, const int *__restrict__ n_persons, JointBatch b, LrTable lr, int P, int K,
                     float S_w, float S_h, float4 *__restrict__ out, const float2 *__restrict__ noise, JitterBatch jb)
{
    const int n = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= P * K) return;
    const int p = idx / K, k = idx - p * K;
    const size_t base = (size_t)n * P * K;
    const int np = n_persons ? n_persons[n] : P;
    if (p >= np) {                                             // padding rows: copied unchanged
        out[base + idx] = joints[base + idx];
        return;
    }
    int ks = k;                                                // the row that lands in channel k: its mirror partner under a flip
    if (b.flip[n]) {
        for (int i = 0; i < lr.n; ++i) {
            if (lr.left[i] == k) ks = lr.right[i];
            else if (lr.right[i] == k) ks = lr.left[i];
        }
    }
    const float4 j = joints[base + (size_t)p * K + ks];
    const double *M = b.M[n];
    const double x = (double)j.x, y = (double)j.y;
    float4 o;
    o.x = (float)__dadd_rn(__dadd_rn(__dmul_rn(M[0], x), __dmul_rn(M[1], y)), M[2]);
    o.y = (float)__dadd_rn(__dadd_rn(__dmul_rn(M[3], x), __dmul_rn(M[4], y)), M[5]);
    o.w = (float)__dmul_rn((double)j.w, b.scale[n]);
    o.z = (o.x <= 0.f || o.y <= 0.f || o.x > S_w || o.y > S_h) ? 0.f : j.z;   // (a NaN coordinate keeps v, as the reference's comparison does)
    if (noise && jb.gate[n]) {                                 // AnnotationJitter: after the visibility test, the noise of the OUTPUT row
        const float2 u = noise[base + idx];
        o.x = o.x + jb.eps[n] * (((u.x - 0.5f) + jb.shift[n]) * 2.f);
        o.y = o.y + jb.eps[n] * (((u.y - 0.5f) + jb.shift[n]) * 2.f);
    }
    out[base + idx] = o;
}

// |m0| S + |m1| S + |m2| < 2^20 for both rows of every image: what lets the kernel work in int32
bool warp_rows_in_range(const double *D, int n, int S)
{
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 2; ++r) {
            const double *m = D + i * 6 + r * 3;
            const double reach = fabs(m[0]) * S + fabs(m[1]) * S + fabs(m[2]);
            if (!(reach < 1048576.0)) return false;            // (also refuses NaN / inf)
        }
    return true;
}

template <int C, bool NORM, bool PHOTO = false>
int warp_launch(const char *name, const unsigned char *raw, const long *offsets, const int *hw4, int n, const double *D, int S,
                const WarpArgs &a, float *out_f, unsigned char *out_u8, hipStream_t stream, const int *photo4 = nullptr)
{
    OG_REQUIRE(n > 0 && S > 0 && S <= 16384, OG_EINVAL, "%s: bad shape", name);
    for (int i = 0; i < n; ++i)
        OG_REQUIRE(hw4[i * 4] > 0 && hw4[i * 4 + 1] > 0 && (long)hw4[i * 4] * hw4[i * 4 + 1] < (1l << 28) && offsets[i] >= 0, OG_EINVAL,
                   "%s: image %d: bad shape", name, i);
    OG_REQUIRE(warp_rows_in_range(D, n, S), OG_EINVAL, "%s: a source coordinate could reach 2^20 (or D is not finite)", name);
    if constexpr (PHOTO) {
        for (int i = 0; i < n; ++i)
            OG_REQUIRE(photo::desc_ok(photo4 + i * 4), OG_EINVAL, "%s: image %d: bad photometric descriptor", name, i);
    }
    const int tiles_x = (S + kWarpTW - 1) / kWarpTW, tiles_y = (S + kWarpTH - 1) / kWarpTH;
    const size_t align = NORM ? 15 : 3;
    const int vec4 = S % 4 == 0 && ((size_t)(NORM ? (const void *)out_f : (const void *)out_u8) & align) == 0;
    for (int first = 0; first < n; first += kWarpBatchMax) {       // at most kWarpBatchMax descriptors ride in one launch's arguments
        const int m = n - first < kWarpBatchMax ? n - first : kWarpBatchMax;
        WarpBatch b;
        for (int i = 0; i < kWarpBatchMax; ++i) {
            const int j = first + (i < m ? i : 0);
            b.off[i] = offsets[j]; b.h[i] = hw4[j * 4]; b.w[i] = hw4[j * 4 + 1];
            for (int k = 0; k < 6; ++k) b.D[i][k] = D[j * 6 + k];
        }
        PhotoArg<PHOTO> pb;
        if constexpr (PHOTO) {
            for (int i = 0; i < kWarpBatchMax; ++i) {
                const int *p4 = photo4 + (first + (i < m ? i : 0)) * 4;
                pb.d[i] = photo::Desc{p4[0], p4[1], p4[2], p4[3]};
            }
        }
        const size_t plane = (size_t)first * S * S;
        hipLaunchKernelGGL((warp_affine_kernel<C, NORM, PHOTO>), dim3((unsigned)(tiles_x * tiles_y), (unsigned)m), dim3(256), 0, stream,
                           raw, b, a, S, tiles_x, out_f ? out_f + plane * C : nullptr, out_u8 ? out_u8 + plane * (NORM ? C : 1) : nullptr,
                           vec4, pb);
        OG_LAUNCH_CHECK(name);
    }
    return OG_OK;
}

}  // namespace

OG_API int og_warp_affine_batch_u8(const unsigned char *raw, const long *offsets, const int *hw4, int n, const double *D, int S,
                                   const unsigned char *border3, const float *mean3, const float *std3, float *out,
                                   unsigned char *out_u8, void *stream)
{
    const char *name = "og_warp_affine_batch_u8";
    OG_REQUIRE(raw && offsets && hw4 && D && border3 && mean3 && std3 && out, OG_EINVAL, "%s: null pointer", name);
    WarpArgs a;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; a.border[c] = border3[c]; }
    return warp_launch<3, true>(name, raw, offsets, hw4, n, D, S, a, out, out_u8, (hipStream_t)stream);
}

OG_API int og_warp_affine_photo_batch_u8(const unsigned char *raw, const long *offsets, const int *hw4, int n, const double *D, int S,
                                         const unsigned char *border3, const float *mean3, const float *std3, float *out,
                                         unsigned char *out_u8, const int *photo4, void *stream)
{
    const char *name = "og_warp_affine_photo_batch_u8";
    OG_REQUIRE(raw && offsets && hw4 && D && border3 && mean3 && std3 && out && photo4, OG_EINVAL, "%s: null pointer", name);
    WarpArgs a;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; a.border[c] = border3[c]; }
    return warp_launch<3, true, true>(name, raw, offsets, hw4, n, D, S, a, out, out_u8, (hipStream_t)stream, photo4);
}

OG_API int og_warp_affine_mask_u8(const unsigned char *masks, const long *offsets, const int *hw4, int n, const double *D, int S,
                                  int border, unsigned char *out, void *stream)
{
    const char *name = "og_warp_affine_mask_u8";
    OG_REQUIRE(masks && offsets && hw4 && D && out, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(border >= 0 && border <= 255, OG_EINVAL, "%s: border outside [0, 255]", name);
    WarpArgs a = {};
    a.border[0] = border;
    return warp_launch<1, false>(name, masks, offsets, hw4, n, D, S, a, nullptr, out, (hipStream_t)stream);
}

namespace {

// both keypoint entry points: noise == null is the plain transform
int joints_launch(const char *name, const float *joints, const int *n_persons, int N, int P, int K, const double *M, const int *flip,
                  const double *scale, float S_w, float S_h, const int *left, const int *right, int n_lr, const float *noise,
                  const int *gate, const float *eps, const float *shift, float *out, void *stream)
{
    OG_REQUIRE(joints && M && flip && scale && out && (n_lr == 0 || (left && right)), OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && P > 0 && K > 0 && (long)P * K < (1l << 24), OG_EINVAL, "%s: bad shape", name);
    OG_REQUIRE(n_lr >= 0 && n_lr <= kLrMax, OG_EINVAL, "%s: at most %d left / right pairs", name, kLrMax);
    OG_REQUIRE((((size_t)joints | (size_t)out) & 15) == 0, OG_EINVAL, "%s: joints / out not 16-byte aligned", name);
    LrTable lr = {};
    lr.n = n_lr;
    for (int i = 0; i < n_lr; ++i) {
        OG_REQUIRE(left[i] >= 0 && left[i] < K && right[i] >= 0 && right[i] < K, OG_EINVAL, "%s: left / right index outside [0, K)", name);
        lr.left[i] = left[i]; lr.right[i] = right[i];
    }
    for (int first = 0; first < N; first += kWarpBatchMax) {
        const int m = N - first < kWarpBatchMax ? N - first : kWarpBatchMax;
        JointBatch b;
        JitterBatch jb = {};
        for (int i = 0; i < kWarpBatchMax; ++i) {
            const int j = first + (i < m ? i : 0);
            for (int k = 0; k < 6; ++k) b.M[i][k] = M[j * 6 + k];
            b.scale[i] = scale[j]; b.flip[i] = flip[j];
            if (noise) { jb.gate[i] = gate[j]; jb.eps[i] = eps[j]; jb.shift[i] = shift[j]; }
        }
        const size_t rows = (size_t)first * P * K;
        hipLaunchKernelGGL(affine_joints_kernel, dim3((unsigned)((P * K + 255) / 256), (unsigned)m), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4 *>(joints) + rows, n_persons ? n_persons + first : nullptr, b, lr, P, K, S_w, S_h,
                           reinterpret_cast<float4 *>(out) + rows, noise ? reinterpret_cast<const float2 *>(noise) + rows : nullptr, jb);
        OG_LAUNCH_CHECK(name);
    }
    return OG_OK;
}

}  // namespace

OG_API int og_affine_joints_f32(const float *joints, const int *n_persons, int N, int P, int K, const double *M, const int *flip,
                                const double *scale, float S_w, float S_h, const int *left, const int *right, int n_lr, float *out,
                                void *stream)
{
    return joints_launch("og_affine_joints_f32", joints, n_persons, N, P, K, M, flip, scale, S_w, S_h, left, right, n_lr, nullptr, nullptr,
                         nullptr, nullptr, out, stream);
}

OG_API int og_affine_joints_jitter_f32(const float *joints, const int *n_persons, int N, int P, int K, const double *M, const int *flip,
                                       const double *scale, float S_w, float S_h, const int *left, const int *right, int n_lr,
                                       const float *noise, const int *gate, const float *eps, const float *shift, float *out, void *stream)
{
    const char *name = "og_affine_joints_jitter_f32";
    OG_REQUIRE(noise && gate && eps && shift, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(((size_t)noise & 7) == 0, OG_EINVAL, "%s: noise not 8-byte aligned", name);
    return joints_launch(name, joints, n_persons, N, P, K, M, flip, scale, S_w, S_h, left, right, n_lr, noise, gate, eps, shift, out, stream);
}
