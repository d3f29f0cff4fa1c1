// K2 -- LimbsCollect.generate_limbs (decoder/collect.py:62-236, _channel_dets :246-254) as its own launch: one wave
// per (image, limb type) over the (N,C,k) candidate lists of og_nms_topk_f32.  The arithmetic lives in collect_body.h
// (shared with the single-launch og_generate_limbs_f32).  KB-sized, latency-bound: ~40 torch launches in the
// reference, one here.
#include "collect_body.h"

namespace {

template <int ND>
__global__ void __launch_bounds__(64)
collect_limbs_kernel(const float *__restrict__ scores, const int64_t *__restrict__ inds, og_collect::Args a)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = blockIdx.x / a.L, l = blockIdx.x % a.L;
    const int cf = a.jf[l], ct = a.jt[l];
    og_collect::limb_rows<ND, int64_t>(a, n, l, threadIdx.x, scores + ((size_t)n * a.C + cf) * a.K,
                                       inds + ((size_t)n * a.C + cf) * a.K, scores + ((size_t)n * a.C + ct) * a.K,
                                       inds + ((size_t)n * a.C + ct) * a.K, sm);
}

__global__ void __launch_bounds__(64)
collect_limbs_scored_kernel(const float *__restrict__ scores, const int64_t *__restrict__ inds, og_collect::ScoredArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int n = blockIdx.x / a.L, l = blockIdx.x % a.L;
    const int cf = a.jf[l], ct = a.jt[l];
    og_collect::limb_rows<2, int64_t>(a, n, l, threadIdx.x, scores + ((size_t)n * a.C + cf) * a.K,
                                      inds + ((size_t)n * a.C + cf) * a.K, scores + ((size_t)n * a.C + ct) * a.K,
                                      inds + ((size_t)n * a.C + ct) * a.K, sm);
}

}  // namespace

// The launch alone, for the two entry points (csrc/nms_topk.hip), which have validated their descriptor: score_ks > 0 takes the
// scored kernel (2-component offsets) with score_hm = the stride-4 heat maps.
int og_collect_launch(const char *name, const float *scores, const int64_t *inds, int N, int vector_nd, const og_collect::Args &a,
                      const float *score_hm, int score_ks, void *stream)
{
    OG_REQUIRE((long)a.H * a.W < (1l << 31), OG_EINVAL, "%s: plane too large", name);
    OG_REQUIRE(a.K <= 2048, OG_EUNSUPPORTED, "%s: k=%d too large", name, a.K);
    const dim3 grid(N * a.L);
    const size_t lds = (size_t)((a.K + 3) & ~3) * 16;
    if (score_ks > 0) {
        const og_collect::ScoredArgs sa{a, score_hm, score_ks, nullptr};
        hipLaunchKernelGGL(collect_limbs_scored_kernel, grid, dim3(64), lds, (hipStream_t)stream, scores, inds, sa);
    } else {
        auto kern = vector_nd == 2 ? collect_limbs_kernel<2> : collect_limbs_kernel<4>;
        hipLaunchKernelGGL(kern, grid, dim3(64), lds, (hipStream_t)stream, scores, inds, a);
    }
    OG_LAUNCH_CHECK(name);
    return OG_OK;
}
