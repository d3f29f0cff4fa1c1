// Fused training losses (reference models/losses.py:31-58, :141-256), forward value + gradient in
// ONE pass over (pred, gt, mask_miss).
//
// The reference evaluates each loss with boolean-mask gathers (pred[mask], gt[mask],
// isfinite, where, pow, mul, sum): ~6 full-tensor passes forward and as many backward on
// (N,17+38,128,128) maps.  Here a lane reads 16 B of pred/gt (+ the per-pixel mask byte), accumulates
// the masked loss in fp32, writes d(loss)/d(pred) directly, and the sum leaves through one wave
// reduction + one float atomic per wave (sums are order dependent in the last bits, like torch's).
//   focal_l2:  0.5 (s-s*)^2 |1-st|^g,  st = s if s* >= tau else 1-s
//              d/ds = (s-s*) |1-st|^g + 0.5 (s-s*)^2 g |1-st|^(g-1) * d|1-st|/ds
//   offset l1: e = |p-g| / ps, kept if e >= margin; optional sqrt(e)
//              d/dp = sign(p-g)/ps   (x 0.5/sqrt(e) with sqrt)   -- the caller divides by (1+count)
#include <math.h>

#include "og_common.h"

namespace {

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ void __launch_bounds__(256)
focal_l2_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const unsigned char *__restrict__ mask,
                int C, long hw, long total, float tau, float gamma, float *__restrict__ sum, float *__restrict__ grad)
{
    float acc = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / ((long)C * hw), pix = i % hw;
        const float s = pred[i], t = gt[i];
        float g = 0.f;
        if (mask[n * hw + pix] && isfinite(t)) {
            const bool fg = t >= tau;
            const float om = fg ? 1.f - s : s;          // 1 - st
            const float a = fabsf(om);
            const float d = s - t;
            const float f = (gamma == 1.f) ? a : powf(a, gamma);
            acc += 0.5f * d * d * f;
            // d|1-st|/ds = sign(om) * (fg ? -1 : +1)
            const float da = (om > 0.f ? 1.f : (om < 0.f ? -1.f : 0.f)) * (fg ? -1.f : 1.f);
            // |x|^gamma at x = 0: derivative 0 (da = 0), also for gamma < 1 where powf(0, gamma - 1) = inf would make inf * 0 = NaN
            const float df = (gamma == 1.f) ? da : (a > 0.f ? gamma * powf(a, gamma - 1.f) * da : 0.f);
            g = d * f + 0.5f * d * d * df;
        }
        grad[i] = g;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) atomicAdd(sum, acc);
}

__global__ void __launch_bounds__(256)
offset_l1_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ ps,
                 const unsigned char *__restrict__ mask, int C, long hw, long total, float margin, int sqrt_re,
                 float *__restrict__ acc2, float *__restrict__ grad)
{
    float acc = 0.f, cnt = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / ((long)C * hw), pix = i % hw;
        const float p = pred[i], t = gt[i], sc = ps[i];
        float g = 0.f;
        const float tn = t / sc;                        // the reference normalises both sides first
        if (mask[n * hw + pix] && isfinite(tn)) {
            const float d = p / sc - tn;
            const float e = fabsf(d);
            if (e >= margin) {
                const float sg = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) / sc;
                if (sqrt_re) {
                    const float r = sqrtf(e);
                    acc += r;
                    g = sg * 0.5f / r;
                } else {
                    acc += e;
                    g = sg;
                }
                cnt += 1.f;
            }
        }
        grad[i] = g;
    }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { atomicAdd(acc2, acc); atomicAdd(acc2 + 1, cnt); }
}

unsigned loss_grid(long total)
{
    const long blocks = (total + 255) / 256;
    return (unsigned)(blocks < 2048 ? blocks : 2048);
}

}  // namespace

OG_API int og_focal_l2_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw,
                                float tau, float gamma, float *sum, float *grad, void *stream)
{
    const char *name = "og_focal_l2_loss_f32";
    OG_REQUIRE(pred && gt && mask_miss && sum && grad, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && hw > 0, OG_EINVAL, "%s: bad shape", name);
    const long total = (long)N * C * hw;
    hipLaunchKernelGGL(focal_l2_kernel, dim3(loss_grid(total)), dim3(256), 0, (hipStream_t)stream, pred, gt, mask_miss, C, hw,
                       total, tau, gamma, sum, grad);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_offset_l1_loss_f32(const float *pred, const float *gt, const float *gt_ps, const unsigned char *mask_miss, int N,
                                 int C, long hw, float margin, int sqrt_re, float *sum_count, float *grad, void *stream)
{
    const char *name = "og_offset_l1_loss_f32";
    OG_REQUIRE(pred && gt && gt_ps && mask_miss && sum_count && grad, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && hw > 0, OG_EINVAL, "%s: bad shape", name);
    const long total = (long)N * C * hw;
    hipLaunchKernelGGL(offset_l1_kernel, dim3(loss_grid(total)), dim3(256), 0, (hipStream_t)stream, pred, gt, gt_ps, mask_miss,
                       C, hw, total, margin, sqrt_re, sum_count, grad);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

// ---- losses of the optional heads and the remaining loss choices (models/losses.py LossChoice) ----
//   l2:         0.5 (p-g)^2                                  heatmap / background, --hmp-loss l2_loss
//   masked l1:  e = |p-g| >= margin (sqrt)                   keypoint scale (targets NaN outside the patches), jitter offset_l1
//   vector l1:  r = sqrt(dx^2 + dy^2) >= margin (sqrt)       channels (2l, 2l+1) are one vector
//   laplace:    v = logb + r exp(-logb) >= margin (sqrt)     logb (N,L,hw) from the spread head; gradient to pred AND logb
// Same scheme as above (grid-stride, masked fp32 accumulation, gradient written in the same pass, one wave reduction + one float
// atomic per wave and accumulator), but a lane owns V consecutive pixels of one channel: V = 4 (one 16-byte load / store per
// operand, the 4 mask bytes as one dword) when hw % 4 == 0 and every base pointer is 16-byte aligned, else V = 1.  With
// hw % V == 0 a lane's pixels never straddle a channel.  Dropped / masked elements get gradient 0 (also where the torch
// formulation's norm backward makes 0 * inf = NaN next to a non-finite target).
namespace {

template <int V> struct Pack;
template <> struct Pack<1> {
    float v[1];
    __device__ __forceinline__ void load(const float *p) { v[0] = *p; }
    __device__ __forceinline__ void store(float *p) const { *p = v[0]; }
};
template <> struct Pack<4> {
    float v[4];
    __device__ __forceinline__ void load(const float *p)
    {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// the V mask bytes of pixels [m, m + V): bit 8 j of the result is non-zero where pixel j is labelled
template <int V> __device__ __forceinline__ unsigned load_mask(const unsigned char *mask, long m)
{
    if (V == 4) return *reinterpret_cast<const unsigned *>(mask + m);
    return mask[m];
}
template <int V> __device__ __forceinline__ bool labelled(unsigned bits, int j) { return (bits >> (8 * j)) & 0xffu; }

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// MODE 0: l2 (acc2[0] += sum).  MODE 1: masked l1 (acc2[0] += sum, acc2[1] += count).  `units` = N*C*hw / V.
template <int V, int MODE>
__global__ void __launch_bounds__(256)
elementwise_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const unsigned char *__restrict__ mask, int C,
                   long hw, long units, float margin, int sqrt_re, float *__restrict__ acc2, float *__restrict__ grad)
{
    float acc = 0.f, cnt = 0.f;
    for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (long)gridDim.x * blockDim.x) {
        const long i = u * V;
        const long n = i / ((long)C * hw), pix = i % hw;
        Pack<V> p, t, g;
        p.load(pred + i);
        t.load(gt + i);
        const unsigned bits = load_mask<V>(mask, n * hw + pix);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float gj = 0.f;
            if (labelled<V>(bits, j) && isfinite(t.v[j])) {
                const float d = p.v[j] - t.v[j];
                if (MODE == 0) {
                    acc += 0.5f * (d * d);
                    gj = d;
                } else {
                    const float e = fabsf(d);
                    if (e >= margin) {
                        if (sqrt_re) {
                            const float r = sqrtf(e);
                            acc += r;
                            gj = sgn(d) * 0.5f / r;
                        } else {
                            acc += e;
                            gj = sgn(d);
                        }
                        cnt += 1.f;
                    }
                }
            }
            g.v[j] = gj;
        }
        g.store(grad + i);
    }
    acc = wave_sum(acc);
    if (MODE == 1) cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(acc2, acc);
        if (MODE == 1) atomicAdd(acc2 + 1, cnt);
    }
}

// LAPLACE 0: vector l1.  LAPLACE 1: laplace (logb / grad_logb (N,L,hw)).  pred / gt / grad (N,2L,hw); `units` = N*L*hw / V.
template <int V, int LAPLACE>
__global__ void __launch_bounds__(256)
vector_kernel(const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ logb,
              const unsigned char *__restrict__ mask, int L, long hw, long units, float margin, int sqrt_re,
              float *__restrict__ acc2, float *__restrict__ grad, float *__restrict__ grad_logb)
{
    float acc = 0.f, cnt = 0.f;
    for (long u = (long)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (long)gridDim.x * blockDim.x) {
        const long i = u * V;                                   // index into (N,L,hw)
        const long nl = i / hw, pix = i % hw, n = nl / L;
        const long ix = (2 * nl) * hw + pix, iy = ix + hw;      // channel 2l of image n is plane n*2L + 2l = 2 (n*L + l)
        Pack<V> px, py, tx, ty, lb, gx, gy, gl;
        px.load(pred + ix);
        py.load(pred + iy);
        tx.load(gt + ix);
        ty.load(gt + iy);
        if (LAPLACE) lb.load(logb + i);
        const unsigned bits = load_mask<V>(mask, n * hw + pix);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float gxj = 0.f, gyj = 0.f, glj = 0.f;
            const float dx = px.v[j] - tx.v[j], dy = py.v[j] - ty.v[j];
            const float r = sqrtf(dx * dx + dy * dy);
            if (labelled<V>(bits, j) && isfinite(r)) {
                const float inv = LAPLACE ? expf(-lb.v[j]) : 1.f;
                const float v = LAPLACE ? lb.v[j] + r * inv : r;
                if (v >= margin) {                              // false for NaN (a non-finite logb) and for a negative laplace value
                    float k = 1.f;                              // d(kept value) / dv
                    if (sqrt_re) {
                        const float s = sqrtf(v);
                        acc += s;
                        k = 0.5f / s;
                    } else {
                        acc += v;
                    }
                    cnt += 1.f;
                    const float kr = r > 0.f ? k * inv / r : 0.f;          // d/dr, / r for the unit vector; norm'(0) = 0
                    gxj = dx * kr;
                    gyj = dy * kr;
                    if (LAPLACE) glj = k * (1.f - r * inv);
                }
            }
            gx.v[j] = gxj;
            gy.v[j] = gyj;
            gl.v[j] = glj;
        }
        gx.store(grad + ix);
        gy.store(grad + iy);
        if (LAPLACE) gl.store(grad_logb + i);
    }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { atomicAdd(acc2, acc); atomicAdd(acc2 + 1, cnt); }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

OG_API int og_l2_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw, float *sum,
                          float *grad, void *stream)
{
    const char *name = "og_l2_loss_f32";
    OG_REQUIRE(pred && gt && mask_miss && sum && grad, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && hw > 0, OG_EINVAL, "%s: bad shape", name);
    const long total = (long)N * C * hw;
    if (hw % 4 == 0 && aligned16(pred) && aligned16(gt) && aligned16(grad) && aligned16(mask_miss))
        hipLaunchKernelGGL((elementwise_kernel<4, 0>), dim3(loss_grid(total / 4)), dim3(256), 0, (hipStream_t)stream, pred, gt,
                           mask_miss, C, hw, total / 4, 0.f, 0, sum, grad);
    else
        hipLaunchKernelGGL((elementwise_kernel<1, 0>), dim3(loss_grid(total)), dim3(256), 0, (hipStream_t)stream, pred, gt,
                           mask_miss, C, hw, total, 0.f, 0, sum, grad);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_masked_l1_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw,
                                 float margin, int sqrt_re, float *sum_count, float *grad, void *stream)
{
    const char *name = "og_masked_l1_loss_f32";
    OG_REQUIRE(pred && gt && mask_miss && sum_count && grad, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && hw > 0, OG_EINVAL, "%s: bad shape", name);
    const long total = (long)N * C * hw;
    if (hw % 4 == 0 && aligned16(pred) && aligned16(gt) && aligned16(grad) && aligned16(mask_miss))
        hipLaunchKernelGGL((elementwise_kernel<4, 1>), dim3(loss_grid(total / 4)), dim3(256), 0, (hipStream_t)stream, pred, gt,
                           mask_miss, C, hw, total / 4, margin, sqrt_re, sum_count, grad);
    else
        hipLaunchKernelGGL((elementwise_kernel<1, 1>), dim3(loss_grid(total)), dim3(256), 0, (hipStream_t)stream, pred, gt,
                           mask_miss, C, hw, total, margin, sqrt_re, sum_count, grad);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_vector_l1_loss_f32(const float *pred, const float *gt, const unsigned char *mask_miss, int N, int C, long hw,
                                 float margin, int sqrt_re, float *sum_count, float *grad, void *stream)
{
    const char *name = "og_vector_l1_loss_f32";
    OG_REQUIRE(pred && gt && mask_miss && sum_count && grad, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && hw > 0, OG_EINVAL, "%s: bad shape", name);
    OG_REQUIRE(C % 2 == 0, OG_EINVAL, "%s: C = %d channels are not (x, y) pairs", name, C);
    const int L = C / 2;
    const long total = (long)N * L * hw;
    if (hw % 4 == 0 && aligned16(pred) && aligned16(gt) && aligned16(grad) && aligned16(mask_miss))
        hipLaunchKernelGGL((vector_kernel<4, 0>), dim3(loss_grid(total / 4)), dim3(256), 0, (hipStream_t)stream, pred, gt,
                           (const float *)nullptr, mask_miss, L, hw, total / 4, margin, sqrt_re, sum_count, grad, (float *)nullptr);
    else
        hipLaunchKernelGGL((vector_kernel<1, 0>), dim3(loss_grid(total)), dim3(256), 0, (hipStream_t)stream, pred, gt,
                           (const float *)nullptr, mask_miss, L, hw, total, margin, sqrt_re, sum_count, grad, (float *)nullptr);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}

OG_API int og_laplace_loss_f32(const float *pred, const float *gt, const float *logb, const unsigned char *mask_miss, int N, int C,
                               long hw, float margin, int sqrt_re, float *sum_count, float *grad, float *grad_logb, void *stream)
{
    const char *name = "og_laplace_loss_f32";
    OG_REQUIRE(pred && gt && logb && mask_miss && sum_count && grad && grad_logb, OG_EINVAL, "%s: null pointer", name);
    OG_REQUIRE(N > 0 && C > 0 && hw > 0, OG_EINVAL, "%s: bad shape", name);
    OG_REQUIRE(C % 2 == 0, OG_EINVAL, "%s: C = %d channels are not (x, y) pairs", name, C);
    const int L = C / 2;
    const long total = (long)N * L * hw;
    if (hw % 4 == 0 && aligned16(pred) && aligned16(gt) && aligned16(logb) && aligned16(grad) && aligned16(grad_logb) &&
        aligned16(mask_miss))
        hipLaunchKernelGGL((vector_kernel<4, 1>), dim3(loss_grid(total / 4)), dim3(256), 0, (hipStream_t)stream, pred, gt, logb,
                           mask_miss, L, hw, total / 4, margin, sqrt_re, sum_count, grad, grad_logb);
    else
        hipLaunchKernelGGL((vector_kernel<1, 1>), dim3(loss_grid(total)), dim3(256), 0, (hipStream_t)stream, pred, gt, logb,
                           mask_miss, L, hw, total, margin, sqrt_re, sum_count, grad, grad_logb);
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
